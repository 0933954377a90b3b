"""CNNTrainer with --spectral-norm gd on the GPU (config '16', batch 4, fixed seeds).

* Phase equivalence against the stock step: with lr_d = lr_g = 0 the weights never move, so the step the spectral-norm trainer runs
  is the stock step on the weights its scopes materialised.  Those are read out (D's in the D phase, D's in the G phase, G's), loaded
  as plain weights into two stock trainers of the same state, and the losses must agree within the project's parity bound (1e-4
  relative; the same kernel routes are taken, so bit-equality is expected and the deviation printed), the ``weight_orig`` gradients
  with the float64 map ``(G - <G, w_sn> u v^T) / sigma`` of the stock gradients within the house rule.
* Graph replay equals eager, bit for bit, losses, parameters and buffers (u, v included), also with an attention block's plain
  convolutions in the mix; two runs are bit-identical.
* After three steps every layer's materialised weight has its largest singular value (float64 ``svdvals`` on the host) within
  ``1 +- d``, d = the largest deviation of a float64 twin of the power iterations over the same weight versions + the house limit."""
import functools

import pytest
import torch

from oracle.procedural import synthetic_images
from spectral_cases import bwd_formula, limit, rel
from tartangan_amd import backend, functional as TF
from tartangan_amd.models.pluggan import GAN_CONFIGS
from tartangan_amd.trainers.cnn import CNNTrainer

pytestmark = pytest.mark.gpu
STEPS = 3


@pytest.fixture(autouse=True, scope='module')
def hip_backend():
    backend._set_backend_for_testing(None)
    backend.get()


def make(device='cuda', config='16', attention=(), **kw):
    cfg = GAN_CONFIGS[config]._replace(attention=tuple(attention))
    tr = CNNTrainer(CNNTrainer.default_args(config=cfg, batch_size=4, device=device, **kw))
    torch.manual_seed(0)
    tr.build_models()
    return tr


class Recorder:
    """Every materialisation of a trainer's scopes, in order: (network, the weight_orig versions, u | v, sigma, w_sn)."""

    def __init__(self, monkeypatch):
        self.calls = []
        orig = TF._SpectralStore.materialize

        def materialize(store, update):
            before = store.uv.clone()
            orig(store, update)
            self.calls.append(dict(store=store, W=[m.weight_orig.detach().cpu().clone() for m in store.layers], uv_before=before.cpu(),
                                   uv=store.uv.cpu().clone(), sigma=store.sigma.cpu().clone(), w_sn=store.w_sn.cpu().clone()))
        monkeypatch.setattr(TF._SpectralStore, 'materialize', materialize)

    def of(self, net):
        store = TF.spectral_store(net)
        return [c for c in self.calls if c['store'] is store]


def per_layer(store, call):
    """{state_dict stem of the layer: (w_sn, u, v, sigma)} of one recorded materialisation."""
    out, off = {}, 0
    for i, (m, (uo, vo)) in enumerate(zip(store.layers, store.uv_offs)):
        n, rows, cols = m.weight_orig.numel(), m.weight_orig.shape[0], m.weight_orig[0].numel()
        out[id(m)] = (call['w_sn'][off:off + n].view(m.weight_orig.shape), call['uv'][uo:uo + rows], call['uv'][vo:vo + cols], call['sigma'][i])
        off += (n + 3) // 4 * 4
    return out


def plain_state(net, start, mats):
    """The state a stock network loads: ``start`` (the spectral-norm network's state before the step) with every
    weight_orig / u / v triple replaced by the materialised weight."""
    names = {id(m): name for name, m in net.named_modules()}
    sd = {k: v for k, v in start.items() if not k.endswith(('weight_orig', 'weight_u', 'weight_v'))}
    for key, (w_sn, _, _, _) in mats.items():
        sd[names[key] + '.weight'] = w_sn
    return sd


def test_phases_equal_the_stock_step_on_the_materialised_weights(monkeypatch, device='cuda'):
    rec = Recorder(monkeypatch)
    zero = dict(lr_d=0., lr_g=0.)
    sn = make(device, spectral_norm='gd', **zero)
    start = {name: {k: v.detach().cpu().clone() for k, v in getattr(sn, name).state_dict().items()} for name in ('g', 'd', 'target_g')}
    imgs = synthetic_images(4, 16, 7)
    torch.manual_seed(1234)
    logs = sn.train_batch(imgs)
    g_calls, d_calls = rec.of(sn.g), rec.of(sn.d)
    assert len(g_calls) == 1 and len(d_calls) == 2
    assert all(torch.equal(a, b) for a, b in zip(d_calls[0]['W'], d_calls[1]['W']))                # lr = 0: the weights did not move
    g_mat = per_layer(TF.spectral_store(sn.g), g_calls[0])
    d_mats = [per_layer(TF.spectral_store(sn.d), c) for c in d_calls]
    runs = []
    for d_mat in d_mats:                                   # run A: D as in the D phase; run B: D as in the G phase
        stock = make(device, **zero)
        stock.g.load_state_dict(plain_state(sn.g, start['g'], g_mat))
        stock.d.load_state_dict(plain_state(sn.d, start['d'], d_mat))
        torch.manual_seed(1234)
        runs.append((stock, stock.train_batch(imgs)))
    (run_a, logs_a), (run_b, logs_b) = runs
    for name, got, want in (('d_loss', logs['d_loss'], logs_a['d_loss']), ('gp', logs['gp'], logs_a['gp']), ('g_loss', logs['g_loss'], logs_b['g_loss'])):
        dev = abs(got - want) / max(abs(want), 1e-12)
        print(f'SN step {name}: spectral-norm trainer {got:.8f} stock on w_sn {want:.8f} relative deviation {dev:.2e}')
        assert dev <= 1e-4, name
    worst = {}
    for tag, net, stock_net, mats in (('d', sn.d, run_a.d, d_mats[0]), ('g', sn.g, run_b.g, g_mat)):
        names = {id(m): name for name, m in net.named_modules()}
        plain = dict(stock_net.named_parameters())
        for m in TF.spectral_store(net).layers:
            w_sn, u, v, sigma = mats[id(m)]
            G = plain[names[id(m)] + '.weight'].grad.detach().cpu()
            args = (G.reshape(len(u), -1), w_sn.reshape(len(u), -1), u, v, sigma)
            want = bwd_formula(*args, torch.float64)
            e32 = rel(bwd_formula(*args, torch.float32), want)
            e = rel(m.weight_orig.grad.detach().cpu().reshape(len(u), -1), want)
            worst[tag] = max(worst.get(tag, (0, 0)), (e, e32))
            assert e <= limit(e32), (tag, names[id(m)], e, e32)
            assert float(want.abs().max()) > 0
        # the other parameters of the network get their gradients as in the stock step
        scale = max(float(p.grad.abs().max()) for p in plain.values())
        for name, p in net.named_parameters():
            if not name.endswith('weight_orig'):
                assert float((p.grad.cpu().double() - plain[name].grad.cpu().double()).abs().max()) <= 1e-4 * scale, (tag, name)
    print(f'SN step weight_orig.grad vs the float64 map of the stock gradients, worst (error, e32): {worst}')


@functools.lru_cache(maxsize=None)
def three_steps(config, attention, graphs, device='cuda', run=0):
    """-> losses of STEPS steps and the final state of g, d, target_g (CPU copies); shared by the tests below."""
    tr = make(device, config, attention, spectral_norm='gd')
    if graphs:
        tr.enable_graphs()
    size = tr.gan_config.base_size * 2 ** len(tr.gan_config.blocks)
    losses = []
    for step in range(STEPS):
        torch.manual_seed(100 + step)
        logs = tr.train_batch(synthetic_images(4, size, 7 + step))
        losses.append((logs['g_loss'], logs['d_loss'], logs['gp']))
    if graphs:
        assert tr._graphs is not None, 'the step did not replay from graphs'
    state = {f'{name}.{k}': v.detach().cpu().clone() for name in ('g', 'd', 'target_g') for k, v in getattr(tr, name).state_dict().items()}
    return losses, state


def same_bits(a, b):
    la, sa = a
    lb, sb = b
    assert la == lb, (la, lb)
    assert sa.keys() == sb.keys()
    for k in sa:
        x, y = sa[k], sb[k]
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), k
    assert any(k.endswith('weight_u') for k in sa) and all(bool(torch.isfinite(v).all()) for v in sa.values() if v.is_floating_point())


@pytest.mark.parametrize('config,attention', [('16', ()), ('32', (2,))])
def test_graph_replay_equals_eager(config, attention):
    same_bits(three_steps(config, attention, False), three_steps(config, attention, True))


def test_two_runs_are_bit_identical():
    same_bits(three_steps('16', (), False), three_steps('16', (), False, run=1))


def test_singular_values_after_three_steps(monkeypatch, device='cuda'):
    rec = Recorder(monkeypatch)
    tr = make(device, spectral_norm='gd')
    for step in range(STEPS):
        torch.manual_seed(100 + step)
        tr.train_batch(synthetic_images(4, 16, 7 + step))
    checked = 0
    for net in (tr.g, tr.d):
        store, calls = TF.spectral_store(net), rec.of(net)
        assert len(calls) == (STEPS if net is tr.g else 2 * STEPS)
        last = per_layer(store, calls[-1])
        # the twin: the same power iterations over the same weight versions, in float64 (and in fp32 on the CPU for e32)
        twin_dev, e32, tops = 0.0, 0.0, {}
        for i, (m, (uo, vo)) in enumerate(zip(store.layers, store.uv_offs)):
            rows, cols = m.weight_orig.shape[0], m.weight_orig[0].numel()
            chains = {}
            for dtype in (torch.float64, torch.float32):
                u, v = calls[0]['uv_before'][uo:uo + rows].to(dtype), calls[0]['uv_before'][vo:vo + cols].to(dtype)
                for c in calls:
                    W = c['W'][i].reshape(rows, cols).to(dtype)
                    v = torch.nn.functional.normalize(torch.mv(W.t(), u), dim=0, eps=1e-12)
                    u = torch.nn.functional.normalize(torch.mv(W, v), dim=0, eps=1e-12)
                    sigma = torch.dot(u, torch.mv(W, v))
                chains[dtype] = float(sigma)
            top = float(torch.linalg.svdvals(calls[-1]['W'][i].reshape(rows, cols).double())[0])
            tops[id(m)] = top
            twin_dev = max(twin_dev, abs(top / chains[torch.float64] - 1))
            e32 = max(e32, abs(chains[torch.float32] - chains[torch.float64]) / abs(chains[torch.float64]))
        d = twin_dev + limit(e32)
        for m in store.layers:
            norm = float(torch.linalg.svdvals(last[id(m)][0].reshape(m.weight_orig.shape[0], -1).double())[0])
            assert 1 - d <= norm <= 1 + d, (norm, d)
            checked += 1
        print(f'SN singular values {"g" if net is tr.g else "d"}: {len(store.layers)} layers, twin deviation {twin_dev:.3e}, e32 {e32:.2e}, d {d:.3e}')
    assert checked > 10
