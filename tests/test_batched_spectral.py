"""The batched spectral-norm route without a GPU, over the emulator (tests/spectral_cases.SpectralEmulator): the entry points'
arithmetic against plain torch, autograd through a spectral scope (R1-style double backward) against a float64 twin, the scope's
lifecycle, the CNN trainer with --spectral-norm gd (launch counts, paired passes, state_dict keys, the target generator's u / v,
strip_spectral_norm, the other trainers' refusal) and two gloo ranks."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F
from torch import nn

from oracle.procedural import synthetic_images
from spectral_cases import EMU, SHAPES, SpectralEmulator, limit, make_layers, reference_bwd, reference_fwd, rel
from tartangan_amd import backend, functional as TF
from tartangan_amd.models.layers import Conv2d, LeakyReLU, SpectralNormConv2d, strip_spectral_norm

EPS = 1e-12


@pytest.fixture(autouse=True)
def emulated_backend():
    prev = backend._set_backend_for_testing(SpectralEmulator())
    yield
    backend._set_backend_for_testing(prev)


# ------------------------------------------------------------------------------------------------ (a) kernel arithmetic
def test_entry_points_against_plain_torch_six_layers_in_one_call():
    layers = make_layers(SHAPES)
    n = len(layers)
    keep = [dict(W=L['W'].clone(), u=L['u'].clone(), v=L['v'].clone(), w_sn=torch.zeros_like(L['W']), g_sn=L['g_sn'].clone(),
                 g_orig=L['g_orig'].clone()) for L in layers]
    items = torch.tensor([[k['W'].data_ptr(), k['u'].data_ptr(), k['v'].data_ptr(), k['w_sn'].data_ptr(), k['g_sn'].data_ptr(),
                           k['g_orig'].data_ptr(), L['rows'], L['cols']] for k, L in zip(keep, layers)], dtype=torch.int64)
    nbytes = EMU.sn_batch_workspace(items, n)
    assert nbytes > 0 and EMU.sn_batch_workspace(items, 0) == 0
    sigma, ws = torch.zeros(n), torch.zeros(nbytes // 4 + 1)
    EMU.sn_batch_fwd(items, n, sigma, ws, nbytes, 1, EPS)
    for i, (k, L) in enumerate(zip(keep, layers)):
        u, v, s, w_sn = reference_fwd(L['W'], L['u'], L['v'], 1, EPS, torch.float64)
        for name, got, want in (('u', k['u'], u), ('v', k['v'], v), ('sigma', sigma[i], s), ('w_sn', k['w_sn'], w_sn)):
            assert rel(got.reshape(-1), want.reshape(-1)) <= 1.2e-7, (L['rows'], L['cols'], name)     # the rounding to fp32 alone
    u_before = [k['u'].clone() for k in keep]
    sigma0 = torch.zeros(n)
    EMU.sn_batch_fwd(items, n, sigma0, ws, nbytes, 0, EPS)               # update = 0: u, v read only, the same sigma again
    assert all(torch.equal(a, k['u']) for a, k in zip(u_before, keep))
    assert rel(sigma0, sigma.double()) <= 2.4e-7
    EMU.sn_batch_bwd(items, n, sigma, ws, nbytes, 1)
    for k, L in zip(keep, layers):
        want = L['g_orig'].double() + reference_bwd(L['W'], k['u'], k['v'], L['g_sn'], torch.float64)
        # autograd through W / dot(u, W v) in float64 against the formula on the fp32-rounded w_sn and sigma: two roundoffs of slack
        assert rel(k['g_orig'], want) <= 4 * 1.2e-7, (L['rows'], L['cols'])
        assert not k['g_sn'].any()                                       # clear = 1


# ------------------------------------------------------------------------------------------------ (b) autograd through a scope
class TwoLayers(nn.Module):
    def __init__(self, conv):
        super().__init__()
        self.convs = nn.Sequential(conv(5, 8, 3, padding=1), LeakyReLU(0.2), conv(8, 6, 1, padding=0))

    def forward(self, x):
        return self.convs(x)


def twin_grads(net, x, dtype):
    """torch autograd in ``dtype`` on a twin that iterates ONCE and then evaluates both forwards with the same W / sigma, u and v
    constants; the loss is R1-style (the input gradient with create_graph, then backward through it)."""
    ws, bs = [], []
    for m in (net.convs[0], net.convs[2]):
        W = m.weight_orig.detach().to(dtype).clone().requires_grad_(True)
        mat = W.reshape(W.shape[0], -1)
        with torch.no_grad():
            v = F.normalize(torch.mv(mat.t(), m.weight_u.to(dtype)), dim=0, eps=EPS)
            u = F.normalize(torch.mv(mat, v), dim=0, eps=EPS)
        ws.append((W, W / torch.dot(u, torch.mv(mat, v))))
        bs.append(m.bias.detach().to(dtype).clone().requires_grad_(True))

    def fwd(inp):
        h = F.leaky_relu(F.conv2d(inp, ws[0][1], bs[0], padding=1), 0.2)
        return F.conv2d(h, ws[1][1], bs[1])
    xa = x.to(dtype).clone().requires_grad_(True)
    ya, yb = fwd(xa), fwd(2 * x.to(dtype))
    g, = torch.autograd.grad(ya.sum(), xa, create_graph=True)
    (ya.pow(2).mean() + yb.pow(2).mean() + g.pow(2).sum()).backward()
    return [w[0].grad for w in ws] + [b.grad for b in bs]


def test_autograd_through_a_scope_with_r1_double_backward():
    torch.manual_seed(5)
    net = TwoLayers(SpectralNormConv2d)
    x = torch.randn(3, 5, 6, 6)
    want = twin_grads(net, x, torch.float64)
    e32 = [rel(a, b) for a, b in zip(twin_grads(net, x, torch.float32), want)]
    with TF.spectral_scope(net):
        xa = x.clone().requires_grad_(True)
        ya, yb = net(xa), net(2 * x)                                     # two forwards, one weight
        g, = torch.autograd.grad(ya.sum(), xa, create_graph=True)
        (ya.pow(2).mean() + yb.pow(2).mean() + g.pow(2).sum()).backward()
        TF.spectral_backward(net)
    got = [net.convs[0].weight_orig.grad, net.convs[2].weight_orig.grad, net.convs[0].bias.grad, net.convs[2].bias.grad]
    for name, a, b, e in zip(('w0', 'w1', 'b0', 'b1'), got, want, e32):
        print(f'SN scope autograd {name}: e32 {e:.2e} got {rel(a, b):.2e} limit {limit(e):.2e}')
        assert rel(a, b) <= limit(e), name


# ------------------------------------------------------------------------------------------------ (c) scope lifecycle
def test_scope_lifecycle_and_the_per_layer_route_outside_it():
    torch.manual_seed(6)
    net = TwoLayers(SpectralNormConv2d)
    twin = TwoLayers(SpectralNormConv2d)
    twin.load_state_dict(net.state_dict())
    x = torch.randn(2, 5, 4, 4)
    keys = list(net.state_dict().keys())
    u0 = net.convs[0].weight_u.clone()
    with TF.spectral_scope(net):
        y1 = net(x)
        u1 = net.convs[0].weight_u.clone()
        y2 = net(x)
        assert torch.equal(net.convs[0].weight_u, u1) and torch.equal(y1, y2)       # no iteration per forward inside a scope
        with TF.spectral_scope(net):                                                # a nested scope for the same network: nothing
            assert torch.equal(net.convs[0].weight_u, u1)
    assert not torch.equal(u0, u1)
    assert list(net.state_dict().keys()) == keys                                   # u, v are views of one flat buffer now: same keys
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    with TF.spectral_scope(net):
        assert not torch.equal(net.convs[0].weight_u, u1)                           # the next scope iterates again
    net.load_state_dict(sd)                                                         # round trip: copied into the views
    assert torch.equal(net.convs[0].weight_u, u1) and torch.equal(net.convs[0].weight_u, sd['convs.0.weight_u'])
    with TF.spectral_scope(net, update=False):                                      # no iteration: sigma from the stored u, v
        assert torch.equal(net.convs[0].weight_u, u1)
    net.eval()
    with TF.spectral_scope(net):                                                    # eval mode: no iteration either
        assert torch.equal(net.convs[0].weight_u, u1)
    # outside a scope: today's behaviour, one iteration per training forward -- the untouched twin does the same from the same state
    net.train()
    net.load_state_dict(twin.state_dict())
    ya, yb = net(x), twin(x)
    assert torch.equal(ya, yb) and torch.equal(net.convs[0].weight_u, twin.convs[0].weight_u)
    ya, yb = net(x), twin(x)
    assert torch.equal(ya, yb) and torch.equal(net.convs[2].weight_v, twin.convs[2].weight_v)


def test_more_than_one_iteration_stays_on_the_per_layer_route():
    torch.manual_seed(7)
    net = nn.Sequential(SpectralNormConv2d(4, 4, 1, n_power_iterations=2))
    assert TF.spectral_store(net) is None
    with TF.spectral_scope(net):
        u = net[0].weight_u.clone()
        net(torch.randn(1, 4, 2, 2))
        assert not torch.equal(u, net[0].weight_u)


# ------------------------------------------------------------------------------------------------ (d) the trainer
class Counting(SpectralEmulator):
    counts = {}

    def _count(self, name):
        Counting.counts[name] = Counting.counts.get(name, 0) + 1

    def sn_batch_fwd(self, *a):
        self._count('sn_batch_fwd')
        return super().sn_batch_fwd(*a)

    def sn_batch_bwd(self, *a):
        self._count('sn_batch_bwd')
        return super().sn_batch_bwd(*a)

    def sn_power_iter(self, *a):
        self._count('sn_power_iter')
        return super().sn_power_iter(*a)


def make_trainer(cls=None, seed=0, **kw):
    from tartangan_amd.trainers.cnn import CNNTrainer
    cls = cls or CNNTrainer
    tr = cls(cls.default_args(config='16', batch_size=4, device='cpu', **kw))
    torch.manual_seed(seed)
    tr.build_models()
    return tr


def test_default_is_none_and_a_stock_trainer_makes_no_spectral_call():
    from tartangan_amd.trainers.cnn import CNNTrainer
    assert CNNTrainer.default_args().spectral_norm == 'none'
    backend._set_backend_for_testing(Counting())
    Counting.counts = {}
    tr = make_trainer()
    torch.manual_seed(1)
    tr.train_batch(synthetic_images(4, 16, 7))
    assert not Counting.counts
    assert not any(isinstance(m, SpectralNormConv2d) for net in (tr.g, tr.d, tr.target_g) for m in net.modules())


def test_trainer_with_spectral_norm_gd():
    backend._set_backend_for_testing(Counting())
    tr = make_trainer(spectral_norm='gd')
    stock = make_trainer()
    # every conv_factory layer, nothing else: the same keys as the stock model wrapped with torch.nn.utils.spectral_norm
    for mine, plain in ((tr.g, stock.g), (tr.d, stock.d)):
        for m in list(plain.modules()):
            if type(m) is Conv2d:
                nn.utils.spectral_norm(m)
        assert list(mine.state_dict().keys()) == list(plain.state_dict().keys())
    assert tr._d_pairable() and tr._g_pairable()
    imgs = synthetic_images(4, 16, 7)
    torch.manual_seed(1)
    for step in range(2):
        Counting.counts = {}
        orig = {k: v.clone() for k, v in tr.d.state_dict().items() if k.endswith('weight_orig')}
        logs = tr.train_batch(imgs)
        assert Counting.counts == dict(sn_batch_fwd=3, sn_batch_bwd=2), (step, Counting.counts)     # D twice, G once; no per-layer call
        assert all(torch.isfinite(torch.tensor(v)) for v in logs.values())
        assert all(not torch.equal(v, tr.d.state_dict()[k]) for k, v in orig.items())                # every weight_orig got a gradient
    g_sd, t_sd = tr.g.state_dict(), tr.target_g.state_dict()
    uv = [k for k in g_sd if k.endswith('weight_u') or k.endswith('weight_v')]
    assert uv and all(torch.equal(g_sd[k], t_sd[k]) for k in uv)
    # stripped: a plain Generator computes what the spectral-norm target generator computes in eval mode
    plain_g = make_trainer().g
    plain_g.load_state_dict(strip_spectral_norm(t_sd))
    assert not any(k.endswith(('weight_orig', 'weight_u', 'weight_v')) for k in strip_spectral_norm(t_sd))
    plain_g.eval()
    tr.target_g.eval()
    z = torch.randn(3, tr.gan_config.latent_dims)
    with torch.no_grad():
        want, got = tr.target_g(z), plain_g(z)
    # two fp32 roundings per filter element (1 / sigma, the product) against one of the float64 quotient, through 8 layers
    assert rel(got, want.double()) <= 1e-5


def test_d_and_g_alone():
    backend._set_backend_for_testing(Counting())
    for flag, want in (('d', dict(sn_batch_fwd=2, sn_batch_bwd=1)), ('g', dict(sn_batch_fwd=1, sn_batch_bwd=1))):
        tr = make_trainer(spectral_norm=flag)
        Counting.counts = {}
        torch.manual_seed(1)
        tr.train_batch(synthetic_images(4, 16, 7))
        assert Counting.counts == want, (flag, Counting.counts)


def test_per_layer_switch_takes_the_old_route():
    backend._set_backend_for_testing(Counting())
    tr = make_trainer(spectral_norm='gd', spectral_per_layer=True)
    Counting.counts = {}
    torch.manual_seed(1)
    tr.train_batch(synthetic_images(4, 16, 7))
    assert Counting.counts.get('sn_power_iter', 0) > 0 and 'sn_batch_fwd' not in Counting.counts


def test_other_trainers_refuse_the_flag():
    from tartangan_amd.trainers.info import InfoTrainer
    from tartangan_amd.trainers.iqn import IQNTrainer
    from tartangan_amd.trainers.scene import SceneTrainer
    from tartangan_amd.trainers.shared.cnn import CNNTrainer as SharedCNNTrainer
    from tartangan_amd.trainers.shared.iqn import IQNTrainer as SharedIQNTrainer
    from tartangan_amd.trainers.text_cnn import TextCNNTrainer
    for cls in (IQNTrainer, SceneTrainer, SharedCNNTrainer, SharedIQNTrainer, InfoTrainer, TextCNNTrainer):
        with pytest.raises(NotImplementedError, match='spectral-norm'):
            cls(cls.default_args(config='16', batch_size=4, device='cpu', spectral_norm='d'))
        cls(cls.default_args(config='16', batch_size=4, device='cpu'))              # 'none': as before


# ------------------------------------------------------------------------------------------------ (e) two gloo ranks
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from tartangan_amd.parallel import DataParallel
    backend._set_backend_for_testing(SpectralEmulator())
    tr = make_trainer(seed=rank, spectral_norm='gd')                    # different init per rank: sync_state must fix it, u and v included
    dp = DataParallel(tr)
    imgs = dp.shard(synthetic_images(8, 16, 4321))
    torch.manual_seed(1234)
    tr.train_batch(imgs)
    state = torch.cat([tr.optimizer_d.flat, tr.optimizer_g.flat, TF.spectral_store(tr.d).uv, TF.spectral_store(tr.g).uv,
                       TF.spectral_store(tr.target_g).uv])
    gathered = [torch.zeros_like(state) for _ in range(world)]
    dist.all_gather(gathered, state)
    if rank == 0:
        out.put(dict(equal=all(torch.equal(gathered[0].view(torch.int32), t.view(torch.int32)) for t in gathered),
                     finite=bool(torch.isfinite(state).all()), n=state.numel()))
    dist.destroy_process_group()


def test_two_gloo_ranks_hold_identical_weights_u_and_v():
    world = 2
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    res = out.get(timeout=300)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res['equal'] and res['finite'] and res['n'] > 0
