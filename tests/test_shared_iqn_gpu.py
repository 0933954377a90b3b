"""The shared-filter IQN trainer end to end on the MI355X: the HIP ``trainers.shared.iqn.IQNTrainer`` (fused head) against the
fixtures the reference's own trainer produced (tests/golden/shared_iqn_*.json), both steps at 1e-4; the step replayed from HIP
graphs against the eager step, bit for bit; the tensors the optimiser must leave alone; and the composed head
(``TG_IQN_FUSED_HEAD=0``) holding the same fixture from a fresh child process."""
import os
import subprocess
import sys

import pytest
import torch

import shared_iqn_cases as SI
from oracle.procedural import summarize, synthetic_images
from tartangan_amd.models.blocks import FusedIQNDiscriminatorOutput
from tartangan_amd.models.shared.blocks import SharedConvBlock

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def hip_backend():
    from tartangan_amd import backend
    backend._set_backend_for_testing(None)
    backend.get()
    yield


def _close(a, b, rel, abs_=1e-6):
    return abs(a - b) <= abs_ + rel * max(abs(a), abs(b))


def _fixture_steps(case, tag):
    """Eager.  Losses, parameter L2s and gradient L2s of BOTH steps at 1e-4; every figure is printed before it is asserted."""
    fx = SI.load_shared_iqn_fixture(case)
    tr = SI.shared_iqn_trainer(fx, 'cuda')
    assert type(tr.d.to_output) is FusedIQNDiscriminatorOutput
    assert list(tr.g.state_dict().keys()) == fx['state_keys']['g']
    assert list(tr.d.state_dict().keys()) == fx['state_keys']['d']
    di = fx['default_init']
    assert _close(SI.total_l2(tr.g), di['g_l2'], 1e-6)
    assert _close(SI.total_l2(tr.target_g), di['target_g_l2'], 1e-6)
    assert _close(SI.total_l2(tr.d), di['d_l2'], 1e-6)
    SI.load_procedural(tr, fx)
    torch.manual_seed(fx['rng_seed'])
    failures = []
    for k, ref in enumerate(fx['steps']):
        logs = tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k))
        got = dict(logs, g_l2=SI.total_l2(tr.g), d_l2=SI.total_l2(tr.d), target_g_l2=SI.total_l2(tr.target_g),
                   g_grad_l2=SI.total_l2(tr.g, True), d_grad_l2=SI.total_l2(tr.d, True))
        for name, want in ref.items():
            rel = abs(got[name] - want) / max(abs(want), 1e-12)
            print(f'{tag} {case} step {k + 1} {name}: hip {got[name]:.7g} reference {want:.7g} rel {rel:.2e}')
            if not _close(got[name], want, 1e-4):
                failures.append((k + 1, name, got[name], want))
        if k == 0:
            for net in ('d', 'g'):
                for name, p in getattr(tr, net).named_parameters():
                    if fx['after_step1'][net + '_grad'][name] is None:      # never given a gradient by the reference: a zero one here
                        assert summarize(p.grad, 4)['max_abs'] == 0.0, (net, name)
    assert not failures, failures
    assert float(torch.rand(1)) == fx['rng_after']          # the z / tau stream consumed like the reference
    z, t = ('z', fx['batch'], fx['latent_dims']), ('tau', fx['num_quantiles'] * fx['batch'], fx['num_quantiles'])
    assert tr.rng_feed.plan == [z, t, t, z, t]


@pytest.mark.parametrize('case', SI.SHARED_IQN_CASES)
def test_hip_shared_iqn_trainer_matches_reference_fixture(case, monkeypatch):
    monkeypatch.delenv('TG_IQN_FUSED_HEAD', raising=False)
    _fixture_steps(case, 'SHARED-IQN')


def test_composed_head_holds_the_same_fixture_in_a_fresh_process():
    """``TG_IQN_FUSED_HEAD=0``: the parent's composed forward, same trainer, same fixture, both steps at 1e-4."""
    code = ('import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); import test_shared_iqn_gpu as T; '
            'from tartangan_amd import backend; backend.get(); T._fixture_steps("shared_iqn_c16_b4", "SHARED-IQN composed"); print("CHILD OK")')
    r = subprocess.run([sys.executable, '-c', code, REPO], env=dict(os.environ, TG_IQN_FUSED_HEAD='0'), cwd=REPO,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and 'CHILD OK' in r.stdout, r.stdout[-4000:]


def test_forward_pins_on_the_device(monkeypatch):
    import copy
    monkeypatch.delenv('TG_IQN_FUSED_HEAD', raising=False)
    fx = SI.load_shared_iqn_fixture('shared_iqn_c32a2_b4')
    tr = SI.shared_iqn_trainer(fx, 'cuda')
    SI.load_procedural(tr, fx)
    B = fx['batch']
    with torch.no_grad():
        g2, d2 = copy.deepcopy(tr.g), copy.deepcopy(tr.d)
        z = torch.randn(B, tr.gan_config.latent_dims, generator=torch.Generator().manual_seed(99)).cuda()
        g_out = g2(z)
        torch.manual_seed(555)
        p_real, loss_real = d2(synthetic_images(B, fx['size'], fx['img_seed']).cuda(), targets=torch.ones(B, 1).cuda())
        p_fake, loss_fake = d2(g_out, targets=torch.zeros(B, 1).cuda())
    ref = fx['forward']['g_out']
    got = summarize(g_out, len(ref['idx']))
    assert _close(got['l2'], ref['l2'], 1e-5)
    for got, name in ((p_real, 'd_real'), (p_fake, 'd_fake')):
        for a, b in zip(got.reshape(-1).tolist(), fx['forward'][name]):
            assert _close(a, b, 1e-4, 1e-5), name
    assert _close(float(loss_real), fx['forward']['d_real_loss'], 1e-4) and _close(float(loss_fake), fx['forward']['d_fake_loss'], 1e-4)


def test_graph_replay_equals_eager_bit_for_bit(monkeypatch):
    """Four calls: record (eager, the draw order z, tau, tau, z, tau is learnt), capture + replay, replay, replay.  The losses of
    every call equal the eager trainer's exactly, and so do both parameter buckets and the host random stream after each call."""
    monkeypatch.delenv('TG_IQN_FUSED_HEAD', raising=False)
    fx = SI.load_shared_iqn_fixture('shared_iqn_c16_b4')
    runs = []
    for graphed in (False, True):
        tr = SI.shared_iqn_trainer(fx, 'cuda')
        SI.load_procedural(tr, fx)
        if graphed:
            tr.enable_graphs()
        torch.manual_seed(fx['rng_seed'])
        calls = []
        for k in range(4):
            logs = tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k).cuda())
            state = torch.get_rng_state()
            calls.append((logs, float(torch.rand(1))))
            torch.set_rng_state(state)               # (peeking must not move the stream the next step draws from)
        runs.append((calls, tr.optimizer_g.flat.clone(), tr.optimizer_d.flat.clone(), getattr(tr, '_graphs', None) is not None))
    eager, graphs = runs
    assert graphs[3] and not eager[3]
    for k, (a, b) in enumerate(zip(eager[0], graphs[0])):
        assert a[0] == b[0], (k, a[0], b[0])
        assert a[1] == b[1], k
    assert torch.equal(eager[1], graphs[1]) and torch.equal(eager[2], graphs[2])
    for name in ('g_loss', 'd_loss', 'gp'):          # and the first step is still the reference's
        assert _close(graphs[0][0][0][name], fx['steps'][0][name], 1e-4)


def test_never_read_columns_and_unused_batchnorm_stay_bit_unchanged_on_the_device(monkeypatch):
    monkeypatch.delenv('TG_IQN_FUSED_HEAD', raising=False)
    fx = SI.load_shared_iqn_fixture('shared_iqn_c16_b4')
    tr = SI.shared_iqn_trainer(fx, 'cuda')
    SI.load_procedural(tr, fx)
    widest = max(fx['blocks'])
    assert tr.g.shared_filters.shape[1] == 100 and widest == 64

    def unused_bn(model):
        first = next(m for m in model.modules() if isinstance(m, SharedConvBlock) and not m.apply_norm)
        return list(first.norm_and_activate.parameters())
    with torch.no_grad():            # the same non-zero values in g and its EMA copy, so that "unchanged" says something
        tr.target_g.shared_filters[:, widest:].copy_(tr.g.shared_filters[:, widest:])
        for p, q in zip(unused_bn(tr.g), unused_bn(tr.target_g)):
            q.copy_(p)
    watched = {}
    for net in ('g', 'd', 'target_g'):
        module = getattr(tr, net)
        watched[(net, 'columns')] = lambda m=module: m.shared_filters[:, widest:]
        for i, p in enumerate(unused_bn(module)):
            watched[(net, f'unused batchnorm {i}')] = lambda p=p: p
    before = {k: get().detach().clone() for k, get in watched.items()}
    assert len(before) == 9 and all(float(v.abs().max()) > 0 for v in before.values())
    torch.manual_seed(fx['rng_seed'])
    for k in range(2):
        tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k))
    for key, get in watched.items():
        assert torch.equal(get().detach().contiguous().view(torch.int32), before[key].contiguous().view(torch.int32)), key
    for net in ('g', 'd'):
        grad = getattr(tr, net).shared_filters.grad
        assert float(grad[:, widest:].abs().max()) == 0.0 and float(grad[:, :widest].abs().min()) > 0.0
