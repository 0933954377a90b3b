"""What happens BETWEEN steps of a trainer that replays from HIP graphs: a batch of another shape, parameter buckets rebuilt
under a live capture, a hyper-parameter changed, a capture that fails, a Parameter object or a whole model replaced.  The
kernels are pinned elsewhere; this pins the host-side state machine that decides which kernels run, on which buffers, with
which constants.

Reference: a trainer that never enables graphs and is never disturbed (or is disturbed by the value-equivalent in-place
operation), given the same seeds and images.  Replay issues the same deterministic kernels on the same inputs, so every
comparison here is BIT EQUALITY -- losses with ``==``, buffers with ``torch.equal`` -- after every step; no tolerance
anywhere in this file."""
import pytest
import torch
from torch import nn

from conftest import load_golden, trainer_from_fixture
from oracle.procedural import procedural_state, synthetic_images

pytestmark = pytest.mark.gpu

CASES = ['c32a2_cnn_b8', 'c32a2_iqn_b8']
IQN = 'c32a2_iqn_b8'


@pytest.fixture(autouse=True)
def hip_backend():
    from tartangan_amd import backend
    backend._set_backend_for_testing(None)
    backend.get()
    yield


def _make(case, graphed):
    fx = load_golden(case)
    tr = trainer_from_fixture(fx, 'cuda')
    tr.g.load_state_dict(procedural_state(tr.g.state_dict(), fx['weight_seed']))
    tr.target_g.load_state_dict(procedural_state(tr.target_g.state_dict(), fx['weight_seed'] + 1))
    tr.d.load_state_dict(procedural_state(tr.d.state_dict(), fx['weight_seed'] + 2))
    if graphed:
        tr.enable_graphs()
    return fx, tr


class Step:
    """One ``train_batch`` call of ``bs`` images; ``before`` / ``after`` are called as ``fn(trainer, role)`` around it, role
    'graphed' or 'control'."""

    def __init__(self, bs=8, before=None, after=None):
        self.bs, self.before, self.after = bs, before, after


def _snapshot(tr, logs):
    snap = dict(logs=dict(logs), step_count=(tr.optimizer_g.step_count, tr.optimizer_d.step_count))
    for name, opt in (('optimizer_g', tr.optimizer_g), ('optimizer_d', tr.optimizer_d)):
        for key in ('flat', 'exp_avg', 'exp_avg_sq'):
            snap[f'{name}.{key}'] = getattr(opt, key).clone()
    for name, net in (('d', tr.d), ('g', tr.g), ('target_g', tr.target_g)):
        for key, value in net.state_dict().items():
            snap[f'{name}.{key}'] = value.clone()
    return snap


def _run(tr, role, fx, steps, seed_offset=0):
    """-> the trainer's complete state after every step, and the host RNG position at the end.  Step k trains on (a slice of)
    the fixture's k-th synthetic batch."""
    torch.manual_seed(fx['rng_seed'] + seed_offset)
    snaps = []
    for k, step in enumerate(steps):
        if step.before is not None:
            step.before(tr, role)
        imgs = synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + seed_offset + k)[:step.bs].cuda()
        snaps.append(_snapshot(tr, tr.train_batch(imgs)))
        if step.after is not None:
            step.after(tr, role)
    return snaps, float(torch.rand(1))


def _assert_identical(got, want):
    (snaps_g, rng_g), (snaps_c, rng_c) = got, want
    assert len(snaps_g) == len(snaps_c)
    for k, (a, b) in enumerate(zip(snaps_g, snaps_c)):
        assert a.keys() == b.keys()
        for name in ('g_loss', 'd_loss', 'gp'):
            assert a['logs'][name] == b['logs'][name], (k, name, a['logs'][name], b['logs'][name])
        assert a['step_count'] == b['step_count'], (k, a['step_count'], b['step_count'])
        for key in a:
            if key not in ('logs', 'step_count'):
                assert torch.equal(a[key], b[key]), (k, key, float((a[key].double() - b[key].double()).abs().max()))
    assert rng_g == rng_c


def _compare(graphed, control, fx, steps, seed_offset=0):
    got = _run(graphed, 'graphed', fx, steps, seed_offset)
    _assert_identical(got, _run(control, 'control', fx, steps, seed_offset))
    return got


@pytest.fixture(scope='module', params=CASES)
def shared_pair(request):
    """One graphed trainer and one control per fixture for the scenarios that need no recapture: the graphs are captured
    once.  Every scenario puts both trainers back to the fixture's start first (``_restart``), so none depends on which
    scenarios ran before it."""
    from tartangan_amd import backend
    backend._set_backend_for_testing(None)
    fx, graphed = _make(request.param, True)
    _, control = _make(request.param, False)
    return fx, graphed, control


def _restart(tr, fx):
    """Put a (possibly graphed) trainer back to the fixture's start IN PLACE -- weights and BatchNorm buffers copied into the
    live buckets, Adam moments and step counts zeroed, learning rates as built -- so that a scenario on the shared pair
    starts from the same state whatever ran before it (another scenario, or none when one test is selected)."""
    tr.g.load_state_dict(procedural_state(tr.g.state_dict(), fx['weight_seed']))
    tr.target_g.load_state_dict(procedural_state(tr.target_g.state_dict(), fx['weight_seed'] + 1))
    tr.d.load_state_dict(procedural_state(tr.d.state_dict(), fx['weight_seed'] + 2))
    for opt, lr in ((tr.optimizer_g, tr.args.lr_g), (tr.optimizer_d, tr.args.lr_d)):
        opt.load_state_dict(dict(step=0, lr=lr, exp_avg=torch.zeros_like(opt.exp_avg), exp_avg_sq=torch.zeros_like(opt.exp_avg_sq)))


def _graph_ids(tr):
    return tuple(id(g) for g in tr._graphs)


def test_ragged_batch_between_replays_runs_eagerly_and_keeps_the_graphs(shared_pair):
    """8, 8, 5, 8, 8 images: the 5-image call has another shape than the recorded RNG plan and the captured graphs, runs
    eagerly (inline draws), and the next full batch replays the SAME graph objects."""
    fx, graphed, control = shared_pair
    _restart(graphed, fx), _restart(control, fx)
    seen = dict(replays=[], graphs=[])
    orig_replay = torch.cuda.CUDAGraph.replay

    def counting_replay(self):
        seen['count'] += 1
        return orig_replay(self)

    def before(tr, role):
        seen['count'] = 0

    def after(tr, role):
        if role == 'graphed':
            seen['replays'].append(seen['count'])
            seen['graphs'].append((tr._graphs, _graph_ids(tr)))

    steps = [Step(bs, before, after) for bs in (8, 8, 5, 8, 8)]
    torch.cuda.CUDAGraph.replay = counting_replay
    try:
        _compare(graphed, control, fx, steps, seed_offset=100)
    finally:
        torch.cuda.CUDAGraph.replay = orig_replay
    assert seen['replays'] == [3, 3, 0, 3, 3]                        # (three graphs per step on one GPU; none for the ragged call)
    assert all(g is seen['graphs'][0][0] and ids == seen['graphs'][0][1] for g, ids in seen['graphs'])     # nothing recaptured
    assert getattr(control, '_graphs', None) is None                 # (the control never had any)


def test_hyper_parameter_change_reaches_the_replayed_step(shared_pair):
    """lr of both optimisers halved after step 2, on both trainers: the six-float hyper buffer is re-uploaded every step and
    nothing is baked into the graphs, so no recapture and the same numbers."""
    fx, graphed, control = shared_pair
    _restart(graphed, fx), _restart(control, fx)

    def halve(tr, role):
        tr.optimizer_d.lr *= 0.5
        tr.optimizer_g.lr *= 0.5

    seen = []

    def graphs(tr, role):
        if role == 'graphed':
            seen.append(tr._graphs)

    steps = [Step(after=graphs), Step(), Step(before=halve), Step(), Step(after=graphs)]
    lr_before = (graphed.optimizer_d.lr, graphed.optimizer_g.lr)
    _compare(graphed, control, fx, steps, seed_offset=200)
    assert seen[0] is not None and seen[1] is seen[0]                # nothing recaptured
    for tr in (graphed, control):
        assert (tr.optimizer_d.lr, tr.optimizer_g.lr) == (lr_before[0] / 2, lr_before[1] / 2)
    # and the halved rate is what the last replayed step was handed (beta1 = 0: the bias correction of lr is exactly 1)
    assert float(graphed.optimizer_d._hyper_host[0]) == float(torch.tensor(graphed.optimizer_d.lr, dtype=torch.float32))


@pytest.mark.parametrize('how', ['grad_none', 'to_cpu_and_back'])
@pytest.mark.parametrize('case', CASES)
def test_buckets_rebuilt_under_a_live_capture_recapture_and_keep_every_value(case, how):
    """After step 2 the discriminator's parameters are detached from the flat buckets from outside -- ``p.grad = None`` (a
    foreign ``zero_grad(set_to_none=True)``), or ``d.to('cpu'); d.to('cuda')``.  Both preserve every value, so the control is
    left alone.  ``ensure_bound`` re-homes the parameters (generation up), the stale graphs are dropped and recaptured, and
    weights, BatchNorm buffers and Adam moments continue bit for bit."""
    fx, graphed = _make(case, True)
    _, control = _make(case, False)
    seen = {}

    def disturb(tr, role):
        if role != 'graphed':
            return
        seen['generation'] = (tr.optimizer_d.generation, tr.optimizer_g.generation)
        seen['graphs'] = tr._graphs
        if how == 'grad_none':
            for p in tr.d.parameters():
                p.grad = None
        else:
            tr.d.to('cpu')
            tr.d.to('cuda')

    _compare(graphed, control, fx, [Step(), Step(), Step(before=disturb), Step(), Step()])
    assert seen['graphs'] is not None
    assert graphed.optimizer_d.generation == seen['generation'][0] + 1
    assert graphed.optimizer_g.generation == seen['generation'][1]              # the generator was not touched
    assert graphed._graphs is not None and graphed._graphs is not seen['graphs']
    assert all(new is not old for new, old in zip(graphed._graphs, seen['graphs']) if new is not None)


def _fail_first_capture_of_g_phase(tr, exc):
    """The first ``_g_phase`` call made while the stream is capturing raises ``exc``: a plain Python exception, no device call
    and nothing done to the stream (``torch.cuda.graph.__exit__`` ends the capture normally)."""
    orig, fired = tr._g_phase, []

    def g_phase(bs):
        if not fired and torch.cuda.is_current_stream_capturing():
            fired.append(True)
            raise exc
        return orig(bs)

    tr._g_phase = g_phase
    return fired


@pytest.mark.parametrize('case', CASES)
def test_capture_failure_falls_back_to_a_correct_eager_step(case):
    """The capture is refused half way (the D-phase graph is already recorded, none has run).  The trainer warns, gives up on
    graphs, and THAT call and every later one are the eager step: nothing that was first created while the stream was
    capturing -- the cached label tensor above all, whose fill was recorded and never executed -- may be read afterwards."""
    fx, graphed = _make(case, True)
    _, control = _make(case, False)
    fired = _fail_first_capture_of_g_phase(graphed, RuntimeError('injected: not permitted while the stream is capturing'))
    seen = {}

    def after_first(tr, role):
        if role == 'graphed':
            seen['requested'], seen['graphs'] = tr._graph_requested, tr._graphs
            seen['labels'] = tr._labels(8).clone()

    steps = [Step(after=after_first)] + [Step() for _ in range(4)]
    with pytest.warns(UserWarning, match='capture failed'):
        got = _run(graphed, 'graphed', fx, steps)
    assert fired == [True]
    assert seen['requested'] is False and seen['graphs'] is None
    # uninitialised memory may happen to be zero: the ones of the first half are the telling part
    assert seen['labels'].shape == (16, 1)
    assert torch.equal(seen['labels'][:8], torch.ones(8, 1, device='cuda'))
    assert torch.equal(seen['labels'][8:], torch.zeros(8, 1, device='cuda'))
    _assert_identical(got, _run(control, 'control', fx, steps))
    assert graphed._graphs is None and graphed._graph_requested is False


def test_kernel_error_during_capture_propagates():
    """A failed tg_* call is a real error wherever it happens: never downgraded to the eager fallback."""
    from tartangan_amd import backend
    fx, graphed = _make(IQN, True)
    fired = _fail_first_capture_of_g_phase(graphed, backend.KernelError('injected: tg_conv2d_fwd failed while the stream is capturing'))
    torch.manual_seed(fx['rng_seed'])
    with pytest.raises(backend.KernelError, match='injected'):
        graphed.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed']).cuda())
    assert fired == [True]
    assert graphed._graphs is None and graphed._graph_requested is True and graphed.steps == 0


def _stride2_conv_deep_in_d(tr):
    """The 3x3 convolution in front of the average pool of the LAST residual block of D (its filter also has derived
    stride-2 layouts that are remembered per module: one more thing that must not go stale)."""
    from tartangan_amd.models.blocks import ResidualDiscriminatorBlock
    block = [m for m in tr.d.blocks if isinstance(m, ResidualDiscriminatorBlock)][-1]
    conv = block.convs[len(block.convs) - 2]
    assert tuple(conv.weight.shape[2:]) == (3, 3)
    return conv


def test_replaced_parameter_object_is_rehomed_at_the_next_step():
    """``conv.weight = nn.Parameter(conv.weight.detach() * 0.5)`` deep inside D after step 2; the control scales the same
    weight in place.  From the very next step on the new object is trained (a view of the bucket), the graphs are
    recaptured, and both runs agree bit for bit."""
    from tartangan_amd.optim import _is_bound
    fx, graphed = _make(IQN, True)
    _, control = _make(IQN, False)
    seen = {}

    def replace(tr, role):
        conv = _stride2_conv_deep_in_d(tr)
        if role == 'graphed':
            seen['generation'], seen['graphs'] = tr.optimizer_d.generation, tr._graphs
            conv.weight = nn.Parameter(conv.weight.detach() * 0.5)
            seen['new'] = conv.weight
        else:
            with torch.no_grad():
                conv.weight.mul_(0.5)

    def rehomed(tr, role):
        if role == 'graphed':
            opt, w = tr.optimizer_d, _stride2_conv_deep_in_d(tr).weight
            assert w is seen['new'] and any(p is w for p in tr.d.parameters())
            assert _is_bound(list(tr.d.parameters()), opt.flat, opt.grads)
            lo, hi = opt.flat.data_ptr(), opt.flat.data_ptr() + 4 * opt.flat.numel()
            assert lo <= w.data_ptr() < hi and w.grad is not None
            assert opt.grads.data_ptr() <= w.grad.data_ptr() < opt.grads.data_ptr() + 4 * opt.grads.numel()
            assert opt.generation == seen['generation'] + 1

    _compare(graphed, control, fx, [Step(), Step(), Step(before=replace, after=rehomed), Step(after=rehomed), Step()])
    assert graphed._graphs is not None and graphed._graphs is not seen['graphs']


def test_pickled_discriminator_carries_no_cache_and_trains_on(tmp_path):
    """``torch.save(tr.d)`` / ``torch.load`` (what the checkpoint component does with whole models) after step 2: the file
    holds no cached parameter list, and the loaded module -- handed to a fresh FusedAdam that takes over the old one's state,
    and put in the live, graphed trainer's place -- trains on exactly like the undisturbed control (the graphs, which have
    the OLD module's buffers baked in, are recaptured)."""
    from tartangan_amd.optim import FusedAdam
    fx, graphed = _make(IQN, True)
    _, control = _make(IQN, False)
    seen = {}

    def swap(tr, role):
        if role != 'graphed':
            return
        path = f'{tmp_path}/d.pt'
        torch.save(tr.d, path)
        back = torch.load(path, weights_only=False)
        assert all('_tg_params' not in m.__dict__ for m in back.modules())
        assert all(m.default_resampling() for m in back.modules() if hasattr(m, 'default_resampling'))    # (fused paths kept)
        assert all('_tg_params' not in m.__dict__ for m in tr.d.modules())
        old = tr.optimizer_d
        opt = FusedAdam(back, lr=old.lr, betas=old.betas, eps=old.eps)
        opt.load_state_dict(old.state_dict())
        seen['graphs'], seen['old_d'] = tr._graphs, tr.d
        tr.d, tr.optimizer_d = back, opt

    _compare(graphed, control, fx, [Step(), Step(), Step(before=swap), Step(), Step()])
    assert graphed.d is not seen['old_d']
    assert graphed._graphs is not None and graphed._graphs is not seen['graphs']
