"""The InfoGAN trainer end to end on the MI355X: the HIP ``trainers.info.InfoTrainer`` against the fixtures the reference's own
trainer produced (tests/golden/info_*.json), both steps at 1e-4; the step replayed from HIP graphs against the eager step, bit
for bit; and the five-key result from one read-back."""
import numpy as np
import pytest
import torch

import info_cases as IC
from oracle.procedural import synthetic_images

pytestmark = pytest.mark.gpu
KEYS = ('g_loss', 'g_code_loss', 'd_loss', 'd_code_loss', 'gp')


@pytest.fixture(autouse=True)
def hip_backend():
    from tartangan_amd import backend
    backend._set_backend_for_testing(None)
    backend.get()
    yield


def _close(a, b, rel, abs_=1e-6):
    return abs(a - b) <= abs_ + rel * max(abs(a), abs(b))


def _images(fx, k):
    return synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k)


@pytest.mark.parametrize('case', IC.INFO_CASES)
def test_hip_info_trainer_matches_reference_fixture(case):
    """Eager.  The five logs, parameter L2s and gradient L2s of BOTH steps at 1e-4; every figure is printed before it is asserted."""
    fx = IC.load_info_fixture(case)
    tr = IC.info_trainer(fx, 'cuda')
    assert list(tr.g.state_dict().keys()) == fx['state_keys']['g']
    assert list(tr.d.state_dict().keys()) == fx['state_keys']['d']
    di = fx['default_init']
    assert _close(IC.total_l2(tr.g), di['g_l2'], 1e-6)
    assert _close(IC.total_l2(tr.target_g), di['target_g_l2'], 1e-6)
    assert _close(IC.total_l2(tr.d), di['d_l2'], 1e-6)
    IC.load_procedural(tr, fx)
    IC.seed_step_streams(fx)
    reads, failures = [], []
    tr._read_back = lambda vals, _rb=tr._read_back: (reads.append(tuple(vals.shape)), _rb(vals))[-1]
    for k, ref in enumerate(fx['steps']):
        logs = tr.train_batch(_images(fx, k))
        assert tuple(logs) == KEYS
        got = IC.step_entry(tr, logs)
        for name, want in ref.items():
            rel = abs(got[name] - want) / max(abs(want), 1e-12)
            print(f'INFO {case} step {k + 1} {name}: hip {got[name]:.7g} reference {want:.7g} rel {rel:.2e}')
            if not _close(got[name], want, 1e-4):
                failures.append((k + 1, name, got[name], want))
    assert not failures, failures
    assert reads == [(5,)] * len(fx['steps'])                 # the five keys from ONE device-to-host read per step
    # both host streams consumed like the reference
    assert dict(torch=float(torch.rand(1)), numpy=float(np.random.rand())) == fx['rng_after']


def test_graph_replay_equals_eager_bit_for_bit():
    """Four calls.  The stock models' draw order (zc, zc) is known in advance: the first call captures and replays, calls 2..4
    replay.  The five losses of every call equal the eager trainer's exactly, and so do the parameter buckets and both host
    random streams after each call."""
    fx = IC.load_info_fixture('info_c16_b4')
    runs = []
    for graphed in (False, True):
        tr = IC.info_trainer(fx, 'cuda')
        IC.load_procedural(tr, fx)
        if graphed:
            tr.enable_graphs()
        IC.seed_step_streams(fx)
        calls = []
        for k in range(4):
            logs = tr.train_batch(_images(fx, k).cuda())
            state, np_state = torch.get_rng_state(), np.random.get_state()
            calls.append((logs, float(torch.rand(1)), float(np.random.rand())))
            torch.set_rng_state(state)               # (peeking must not move the streams the next step draws from)
            np.random.set_state(np_state)
        runs.append((calls, tr.optimizer_g.flat.clone(), tr.optimizer_d.flat.clone(), getattr(tr, '_graphs', None) is not None))
        assert tr.rng_feed.plan == [('zc', fx['batch'], tr.gan_config.latent_dims)] * 2
    eager, graphs = runs
    assert graphs[3] and not eager[3]
    for k, (a, b) in enumerate(zip(eager[0], graphs[0])):
        assert tuple(b[0]) == KEYS and a[0] == b[0], (k, a[0], b[0])
        assert a[1:] == b[1:], k
    assert torch.equal(eager[1], graphs[1]) and torch.equal(eager[2], graphs[2])
    for name in KEYS:                                # and the first step is still the reference's
        assert _close(graphs[0][0][0][name], fx['steps'][0][name], 1e-4)


def test_without_codes_the_entries_are_plain_zeros():
    fx = IC.load_info_fixture('info_c16_b4')
    fx = dict(fx, flags=dict(info_cat_dims=0, info_cont_dims=0, info_w=1.))
    tr = IC.info_trainer(fx, 'cuda')
    torch.manual_seed(fx['rng_seed'])
    logs = tr.train_batch(_images(fx, 0))
    assert tuple(logs) == KEYS and logs['g_code_loss'] == 0. and logs['d_code_loss'] == 0. and logs['gp'] > 0
