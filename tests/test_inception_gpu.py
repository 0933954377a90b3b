"""The Inception-v3 kernels (csrc/inception.hip) and the native network on the GPU, against stock torch in float64 under the
project's "no worse than plain fp32" rule (second_order_cases.errors / violations; the fp32 comparand is torch on the CPU)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_cases as IC
from second_order_cases import errors, violations

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    yield backend.get()
    backend._set_backend_for_testing(prev)


def _pack(w, k):
    """OIHW float32 CPU filter -> the kernel's K-major padded layout (include/tartangan_amd.h)."""
    cout, kk = w.shape[0], w[0].numel()
    wp = torch.zeros(-(-kk // 16) * 16, -(-cout // 128) * 128)
    wp[:kk, :cout] = w.reshape(cout, kk).t()
    assert wp.numel() == k.inception_conv_weight_floats(w.shape[1], cout, w.shape[2], w.shape[3])
    return wp.contiguous()


# (tag, B, Cin, Cout, H, W, KH, KW, stride, ph, pw): every (kernel, stride, padding) combination of the network at that
# layer's real channel counts and plane, batch 2; then the ragged ones
CONV_CASES = [
    ('1a_3x3s2_cin3', 2, 3, 32, 299, 299, 3, 3, 2, 0, 0),
    ('2a_3x3', 2, 32, 32, 149, 149, 3, 3, 1, 0, 0),
    ('2b_3x3p1', 2, 32, 64, 147, 147, 3, 3, 1, 1, 1),
    ('3b_1x1_cout80', 2, 64, 80, 73, 73, 1, 1, 1, 0, 0),
    ('4a_3x3_cin80', 2, 80, 192, 73, 73, 3, 3, 1, 0, 0),
    ('5b_5x5p2_cin48', 2, 48, 64, 35, 35, 5, 5, 1, 2, 2),
    ('5b_3x3p1_cout96', 2, 64, 96, 35, 35, 3, 3, 1, 1, 1),
    ('6a_3x3s2', 2, 288, 384, 35, 35, 3, 3, 2, 0, 0),
    ('6b_1x7', 2, 128, 128, 17, 17, 1, 7, 1, 0, 3),
    ('6b_7x1', 2, 128, 192, 17, 17, 7, 1, 1, 3, 0),
    ('6c_1x7_160', 2, 160, 160, 17, 17, 1, 7, 1, 0, 3),
    ('6b_1x1_768', 2, 768, 192, 17, 17, 1, 1, 1, 0, 0),
    ('7a_3x3s2_cout320', 2, 192, 320, 17, 17, 3, 3, 2, 0, 0),
    ('7b_1x3', 2, 384, 384, 8, 8, 1, 3, 1, 0, 1),
    ('7b_3x1', 2, 384, 384, 8, 8, 3, 1, 1, 1, 0),
    ('7b_3x3p1_cin448', 2, 448, 384, 8, 8, 3, 3, 1, 1, 1),
    ('7c_1x1_cout448_b1', 1, 2048, 448, 8, 8, 1, 1, 1, 0, 0),
    ('ragged_b1_plane', 1, 3, 80, 37, 41, 3, 3, 2, 0, 0),
    ('ragged_big_tiles', 3, 5, 130, 120, 131, 3, 3, 1, 1, 1),       # 128 x 128 tiles with a ragged M, N and K
    ('ragged_pad_wide', 2, 7, 9, 6, 5, 1, 7, 1, 0, 3),
]


def _conv_case(K, case, x_ctot=None, x_coff=0, y_ctot=None, y_coff=0, relu=1, seed=0):
    tag, B, Cin, Cout, H, W, KH, KW, stride, ph, pw = case
    x_ctot, y_ctot = x_ctot or Cin, y_ctot or Cout
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, KH, KW, generator=gen) * (2.0 / (Cin * KH * KW)) ** 0.5
    bias = torch.randn(Cout, generator=gen) * 0.2

    def ref(dtype):
        r = F.conv2d(x.to(dtype), w.to(dtype), bias.to(dtype), stride=stride, padding=(ph, pw))
        return (F.relu(r) if relu else r).double()
    r64, r32 = ref(torch.float64), ref(torch.float32)
    OH, OW = r64.shape[2:]
    xb = torch.full((B, x_ctot, H, W), NAN)
    xb[:, x_coff:x_coff + Cin] = x
    yb = torch.full((B, y_ctot, OH, OW), NAN, device=DEV)
    assert K.inception_conv_supported(B, Cin, Cout, H, W, KH, KW, stride, ph, pw, x_ctot, y_ctot) == 1
    K.inception_conv_fwd(xb.to(DEV), _pack(w, K).to(DEV), bias.to(DEV), yb, B, Cin, Cout, H, W, KH, KW, stride, ph, pw, relu,
                         x_ctot, x_coff, y_ctot, y_coff)
    yb = yb.cpu()
    got = yb[:, y_coff:y_coff + Cout].double()
    outside = torch.cat([yb[:, :y_coff], yb[:, y_coff + Cout:]], 1)
    assert torch.isnan(outside).all(), f'{tag}: wrote outside its channel slice'
    assert torch.isfinite(got).all(), f'{tag}: read outside its channel slice (or left elements unwritten)'
    errs = errors({'y': got}, {'y': r64}, {'y': r32})
    print(tag, 'e_op %.2e e_32 %.2e max %.2e max_32 %.2e' % errs['y'][:4])
    return violations(errs)


@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_against_float64(K, case):
    assert not _conv_case(K, case)


@pytest.mark.parametrize('case', [CONV_CASES[5], CONV_CASES[8], CONV_CASES[12], CONV_CASES[18]], ids=lambda c: c[0])
def test_conv_channel_slices(K, case):
    """NaN outside both slices: the input slice is all that is read, the output slice all that is written."""
    Cin, Cout = case[2], case[3]
    assert not _conv_case(K, case, x_ctot=Cin + 37, x_coff=16, y_ctot=Cout + 45, y_coff=32, seed=1)
    assert not _conv_case(K, case, x_ctot=Cin + 3, x_coff=3, y_ctot=Cout + 1, y_coff=0, relu=0, seed=2)


def test_conv_bad_arguments(K):
    from tartangan_amd.backend import KernelError
    x = torch.zeros(1, 4, 8, 8, device=DEV)
    wp = torch.zeros(K.inception_conv_weight_floats(4, 4, 3, 3), device=DEV)
    y = torch.zeros(1, 4, 6, 6, device=DEV)
    with pytest.raises(KernelError, match='-1'):
        K.inception_conv_fwd(x, wp, None, y, 1, 4, 4, 8, 8, 3, 3, 1, 0, 0, 1, 4, 1, 4, 0)       # input slice past x_ctot
    with pytest.raises(KernelError, match='-2'):
        K.inception_conv_fwd(x, wp, None, y, 1, 4, 4, 8, 8, 3, 3, 3, 0, 0, 1, 4, 0, 4, 0)       # stride 3
    assert K.inception_conv_supported(1, 4, 4, 8, 8, 3, 3, 3, 0, 0, 4, 4) == 0
    K.inception_conv_fwd(x, wp, None, y, 1, 4, 4, 8, 8, 3, 3, 1, 0, 0, 0, 4, 0, 4, 0)           # bias is optional
    assert float(y.abs().max()) == 0.0


@pytest.mark.parametrize('B,C,H,W,x_ctot,x_coff,y_ctot,y_coff', [(2, 64, 147, 147, 64, 0, 64, 0), (2, 288, 35, 35, 288, 0, 768, 480),
                                                               (1, 5, 9, 8, 11, 4, 9, 2)])
def test_pools(K, B, C, H, W, x_ctot, x_coff, y_ctot, y_coff):
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(B, C, H, W, generator=gen)
    xb = torch.full((B, x_ctot, H, W), NAN)
    xb[:, x_coff:x_coff + C] = x
    xd = xb.to(DEV)
    # max-pool: exact
    want = F.max_pool2d(x, kernel_size=3, stride=2)
    yb = torch.full((B, y_ctot) + tuple(want.shape[2:]), NAN, device=DEV)
    K.inception_maxpool3s2(xd, yb, B, C, H, W, x_ctot, x_coff, y_ctot, y_coff)
    yb = yb.cpu()
    assert torch.equal(yb[:, y_coff:y_coff + C], want)
    assert torch.isnan(torch.cat([yb[:, :y_coff], yb[:, y_coff + C:]], 1)).all()
    # average pool: divides by 9 at the border too
    r64 = F.avg_pool2d(x.double(), kernel_size=3, stride=1, padding=1)
    r32 = F.avg_pool2d(x, kernel_size=3, stride=1, padding=1).double()
    yb = torch.full((B, y_ctot, H, W), NAN, device=DEV)
    K.inception_avgpool3(xd, yb, B, C, H, W, x_ctot, x_coff, y_ctot, y_coff)
    yb = yb.cpu()
    got = yb[:, y_coff:y_coff + C].double()
    assert torch.isnan(torch.cat([yb[:, :y_coff], yb[:, y_coff + C:]], 1)).all()
    errs = errors({'y': got}, {'y': r64}, {'y': r32})
    assert not violations(errs), violations(errs)
    border = {'y': got[:, :, 0]}, {'y': r64[:, :, 0]}, {'y': r32[:, :, 0]}
    assert not violations(errors(*border))
    ones = torch.ones(1, 1, 4, 4, device=DEV)
    out = torch.empty_like(ones)
    K.inception_avgpool3(ones, out, 1, 1, 4, 4, 1, 0, 1, 0)
    assert abs(float(out[0, 0, 0, 0]) - 4 / 9) < 1e-6 and abs(float(out[0, 0, 0, 1]) - 6 / 9) < 1e-6


# ------------------------------------------------------------------------------------------------------ the whole network
@pytest.fixture(scope='module')
def network(K):
    """Procedural weights, 299 x 299, batch 2: the native network on the GPU and the float64 / fp32 references, once."""
    from tartangan_amd.models.inception import Inception3
    state = IC.procedural_state(0)
    x = IC.procedural_input(2, 299, seed=3)
    ref64 = IC.reference(state, torch.float64)
    IC.check_reference_health(ref64, x)
    r64 = IC.results(ref64, x.double())
    r32 = IC.results(IC.reference(state, torch.float32), x)
    net = Inception3()
    net.load_state_dict(state)
    return net.to(DEV), state, x, r64, r32


def test_whole_network_against_float64(network):
    net, state, x, r64, r32 = network
    got = IC.results(net, x.to(DEV))
    errs = errors(got, r64, r32)
    for k, e in errs.items():
        print(k, 'e_op %.2e e_32 %.2e max %.2e max_32 %.2e' % e[:4])
    assert not violations(errs), violations(errs)


def test_public_path(network, tmp_path):
    from oracle.fid_features import blocky_images
    from tartangan_amd import inception_utils
    net, state, x, r64, r32 = network
    wrap = inception_utils.WrapInception(net).to(DEV)
    s = blocky_images(2, 64, 11)
    with torch.no_grad():
        pool, logits = wrap.forward_samples(s.to(DEV))
        pre = inception_utils.inception_preprocess(s.to(DEV), (299, 299), 2).cpu()
        w64 = IC.reference(state, torch.float64)(pre.double())
        w32 = IC.reference(state, torch.float32)(pre)
    errs = errors({'pool': pool.double().cpu(), 'logits': logits.double().cpu()}, {'pool': w64[0], 'logits': w64[1]},
                  {'pool': w32[0].double(), 'logits': w32[1].double()})
    assert not violations(errs), violations(errs)

    # prepare_inception_metrics(weights=...) end to end: 64 procedural images against procedural moments
    weights = os.path.join(tmp_path, 'inception.pth')
    torch.save(state, weights)
    data = (torch.randn(80, 2048, generator=torch.Generator().manual_seed(4)) * 0.1 + 0.3).double().numpy()
    moments = os.path.join(tmp_path, 'moments.npz')
    np.savez(moments, mu=data.mean(0), sigma=np.cov(data, rowvar=False))
    get = inception_utils.prepare_inception_metrics(moments, DEV, weights=weights)
    seeds = iter(range(100))
    is_mean, is_std, fid = get(lambda: blocky_images(16, 32, next(seeds)).to(DEV), 64, num_splits=4)
    print('IS %.4f +/- %.4f FID %.4f' % (is_mean, is_std, fid))
    assert np.isfinite([is_mean, is_std, fid]).all() and is_mean >= 1.0 - 1e-5


def test_determinism_capture_and_memory(network):
    net, state, x, r64, r32 = network
    xd = x.to(DEV)
    with torch.no_grad():
        feat = net.features(xd).clone()
        pool, logits = (t.clone() for t in net(xd))
        assert torch.equal(net.features(xd), feat)
        again = net(xd)
        assert torch.equal(again[0], pool) and torch.equal(again[1], logits)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for _ in range(10):
            net(xd)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        # captured and replayed: the same bits as eager
        static = xd.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            gp, gl = net(static)
        gp.zero_(); gl.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gp, pool) and torch.equal(gl, logits)
        static.copy_(xd.flip(0))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gp, pool.flip(0)) and torch.equal(gl, logits.flip(0))
