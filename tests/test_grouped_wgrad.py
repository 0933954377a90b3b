"""Host logic of the grouped 1x1 weight gradients on CPU: inside ``functional.deferred_wgrad()`` a 1x1 layer (and the theta / phi / g
projections of an attention block) launches nothing at the time of the call -- its stage 1 runs in ONE
``conv1x1_wgrad_partials_batch`` at the flush, in front of the reduce rounds.  A backend without that entry point keeps the
per-layer sequence of calls.  (The kernels themselves: tests/test_grouped_wgrad_gpu.py.)"""
import pytest
import torch

from conftest import load_golden, trainer_from_fixture
from emulator import Emulator
from grouped_wgrad_cases import GroupedEmulator
from oracle.procedural import synthetic_images
from tartangan_amd import backend, functional as TF

# without attention; 64 px with an attention block too wide for the one-pass theta / phi / g form; 32 px with one that takes it
FIXTURES = ['c32_cnn_b16', 'c64a1_cnn_b8', 'c32a2_cnn_b8']
LOGGED = ('conv2d_wgrad', 'conv2d_wgrad_partials', 'conv1x1_multi_wgrad', 'conv1x1_wgrad_partials_batch', 'conv2d_wgrad_reduce_batch',
          's2_wgrad_reduce_batch')


def recording(base):
    """A ``base`` emulator that logs (entry point, ks or None, rows or None, deferred context active) of every weight-gradient call."""
    log = []

    class Recording(base):
        pass

    def wrap(name):
        inner = getattr(base, name)

        def call(self, *a):
            ks = a[9] if name == 'conv2d_wgrad_partials' else a[11] if name == 'conv2d_wgrad' else None
            rows = a[0].clone() if name.endswith('_batch') else None
            log.append((name, ks, rows, TF._DeferredWgrad.active))
            return inner(self, *a)
        return call

    for name in LOGGED:
        if hasattr(base, name):
            setattr(Recording, name, wrap(name))
    return Recording(), log


@pytest.fixture(autouse=True)
def restore_backend():
    prev = backend._set_backend_for_testing(Emulator())
    yield
    backend._set_backend_for_testing(prev)


def run_phase(fx, phase, emulator, deferred=True):
    """One D phase or G phase of the fixture's trainer from seeded state -> the phase's flat gradient bucket."""
    backend._set_backend_for_testing(emulator)
    tr = trainer_from_fixture(fx, 'cpu')
    imgs = synthetic_images(fx['batch'], fx['size'], 7)
    import contextlib
    orig = TF.deferred_wgrad
    if not deferred:
        TF.deferred_wgrad = contextlib.nullcontext
    try:
        torch.manual_seed(1)
        if phase == 'd':
            tr._d_phase(imgs)
            return tr.optimizer_d.grads.clone()
        tr._g_phase(fx['batch'])
        return tr.optimizer_g.grads.clone()
    finally:
        TF.deferred_wgrad = orig


@pytest.mark.parametrize('phase', ['d', 'g'])
@pytest.mark.parametrize('case', FIXTURES)
def test_grouped_stage1_gives_the_default_paths_gradients(case, phase):
    fx = load_golden(case)
    want = run_phase(fx, phase, Emulator(), deferred=False)
    em, log = recording(GroupedEmulator)
    got = run_phase(fx, phase, em)
    # (on the GPU the paths are bit-identical, tests/test_grouped_wgrad_gpu.py; the CPU stand-in's sums differ in the last bit with
    # buffer alignment -- the bound of test_deferred_wgrad_never_reduces_one_gradient_twice_in_a_launch)
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-6), float((got - want).abs().max())
    assert any(name == 'conv1x1_wgrad_partials_batch' for name, *_ in log)


@pytest.mark.parametrize('phase', ['d', 'g'])
@pytest.mark.parametrize('case', FIXTURES)
def test_no_per_layer_1x1_launch_inside_the_context_and_one_batch_call_per_flush(case, phase):
    fx = load_golden(case)
    plain, plain_log = recording(Emulator)
    run_phase(fx, phase, plain)
    had_1x1 = sum(1 for name, ks, _, active in plain_log if active and name == 'conv2d_wgrad_partials' and ks == 1)
    had_qkv = sum(1 for name, _, _, active in plain_log if active and name == 'conv1x1_multi_wgrad')
    assert had_1x1 > 0 and (had_qkv > 0) == (case == 'c32a2_cnn_b8')

    em, log = recording(GroupedEmulator)
    run_phase(fx, phase, em)
    inside = [e for e in log if e[3]]
    assert not [e for e in inside if e[0] == 'conv2d_wgrad_partials' and e[1] == 1]
    assert not [e for e in inside if e[0] == 'conv1x1_multi_wgrad']
    # (non-accumulating calls keep the one-call form, with or without the grouped entry)
    assert [e[:2] for e in inside if e[0] == 'conv2d_wgrad'] == [e[:2] for e in plain_log if e[3] and e[0] == 'conv2d_wgrad']
    assert not [e for e in inside if e[0].endswith('_batch')]                    # the flush runs when the context has been left
    batch = [i for i, e in enumerate(log) if e[0] == 'conv1x1_wgrad_partials_batch']
    reduces = [i for i, e in enumerate(log) if e[0] == 'conv2d_wgrad_reduce_batch']
    assert len(batch) == 1 and batch[0] < min(reduces)                           # one flush per phase: stage 1 first
    rows = log[batch[0]][2]
    assert len(rows) == had_1x1 + had_qkv and int((rows[:, 7] > 0).sum()) == had_qkv
    # every stage-1 row has its reduce row, and no launch reduces one gradient twice
    parts = set(rows[:, 4].tolist())
    reduced = [r for i in reduces for r in log[i][2].tolist()]
    assert parts <= {r[0] for r in reduced}
    for i in reduces:
        dst = log[i][2][:, 1].tolist()
        assert len(dst) == len(set(dst))
    assert len(reduces) == len([e for e in plain_log if e[0] == 'conv2d_wgrad_reduce_batch'])
    assert TF._DeferredWgrad.keep == [] and TF._DeferredWgrad.stage1 == [] and TF._DeferredWgrad.items == []


@pytest.mark.parametrize('phase', ['d', 'g'])
@pytest.mark.parametrize('case', FIXTURES)
def test_fallbacks_issue_the_old_sequence_of_calls(case, phase):
    fx = load_golden(case)
    plain, plain_log = recording(Emulator)                 # a backend without the batch entry
    run_phase(fx, phase, plain)
    assert not any(name == 'conv1x1_wgrad_partials_batch' for name, *_ in plain_log)
    assert any(name == 'conv2d_wgrad_partials' and ks == 1 and active for name, ks, _, active in plain_log)
