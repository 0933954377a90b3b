"""The per-op first- and second-order harness (tests/second_order_cases.py) on the emulator backend: the hand-written
backwards of tartangan_amd.functional and the hand-derived second-order formulas of tests/emulator.py (which the HIP
kernels are checked against) against torch's own autograd in float64.  Then proof that the harness has teeth: wrong
variants of the emulator, one of them wrong only by accuracy, must each be rejected."""
import pytest
import torch

import second_order_cases as SO
from emulator import Emulator
from tartangan_amd import backend


@pytest.fixture(autouse=True)
def emulated_backend():
    prev = backend._set_backend_for_testing(Emulator())
    yield
    backend._set_backend_for_testing(prev)


CASES = SO.ragged_cases() + SO.edge_cases()


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_op_matches_float64_torch_to_first_and_second_order(case):
    errs, bad = SO.run_case(case, 'cpu')
    assert not bad, bad
    if case.data is not None:
        assert any(k.startswith('r1.') for k in errs)


def test_case_table_covers_every_discriminator_op():
    kinds = {c.kind for c in CASES}
    want = {'conv2d_3x3', 'conv2d_1x1', 'compose_rgb', 'pool_conv3x3', 'avg_pool2', 'upconv3x3', 'qkv_projections', 'max_pool2',
            'attention_core', 'scale_add', 'batch_norm_act', 'leaky_relu', 'elu', 'selu', 'tanh', 'bilinear_half',
            'fork_bilinear_half', 'copy_channels', 'sum_hw', 'linear', 'add', 'mul', 'iqn_cos_embed', 'repeat_rows',
            'mean_reps', 'iqn_quantile_huber_loss', 'bce_with_logits', 'sumsq'}
    assert want <= kinds, sorted(want - kinds)
    assert {c.name for c in CASES if c.kind == 'conv2d_3x3' and '+res_up' in c.name}
    r1 = {c.kind for c in CASES if c.data is not None}
    assert {'conv2d_3x3', 'compose_rgb', 'pool_conv3x3', 'qkv_projections', 'max_pool2', 'attention_core', 'batch_norm_act',
            'leaky_relu', 'elu', 'selu', 'bilinear_half', 'fork_bilinear_half', 'linear', 'repeat_rows'} <= r1


@pytest.mark.parametrize('case', [SO.lrelu_zero_case(), SO.bn_zero_case()], ids=lambda c: c.name)
def test_lrelu_derivative_at_exact_zero_is_torchs(case):
    """torch: d leaky_relu(x)/dx at x == +0.0 and -0.0 is ``slope``; first order and under the R1 form, exactly."""
    base, cot, r64, r32 = SO.references(case)
    got = SO._evaluate(case.ours, base, case, 'cpu', torch.float32, cot, True)
    for k in r32:
        if k.startswith(('vjp.x', 'r1.x')):
            torch.testing.assert_close(got[k], r32[k], rtol=2e-5, atol=1e-6, msg=k)


# --------------------------------------------------------------------------- the harness has teeth
def _round_mantissa(t, bits=16):
    """``t`` rounded to ``bits`` explicit mantissa bits (nearest): a relative error of ~2^-(bits+1)."""
    drop = 23 - bits
    i = t.contiguous().view(torch.int32)
    r = ((i + (1 << (drop - 1))) & ~((1 << drop) - 1)).view(torch.float32)
    return r.view(t.shape)


class _ScaledAGamma(Emulator):
    def bn_act_dbwd(self, v, vg, vb, gz, x, mean, invstd, gamma, beta, slope, a_gz, a_x, a_gamma, ws, B, C, HW, accumulate=0):
        prev = a_gamma.clone()
        super().bn_act_dbwd(v, vg, vb, gz, x, mean, invstd, gamma, beta, slope, a_gz, a_x, a_gamma, ws, B, C, HW, accumulate)
        base = prev if accumulate else torch.zeros_like(prev)
        a_gamma.copy_(base + (a_gamma - base) * (1 + 1e-3))
        return 0


class _DgradDropsLastChannel(Emulator):
    def conv2d_dgrad(self, gy, w, gx, B, Cin, Cout, H, W, ks):
        g = gy.view(B, Cout, H * W).clone()
        g[:, -1] = 0
        return super().conv2d_dgrad(g, w, gx, B, Cin, Cout, H, W, ks)


class _LReluGeAtZero(Emulator):
    """LeakyReLU derivative 1 at y == 0 (the `>= 0` mask)."""

    @staticmethod
    def _bn_parts(x, mean, invstd, gamma, beta, slope, B, C, HW):
        xhat, y, _ = Emulator._bn_parts(x, mean, invstd, gamma, beta, slope, B, C, HW)
        return xhat, y, torch.where(y >= 0, torch.ones_like(y), torch.full_like(y, slope))

    def lrelu_bwd(self, g, x, slope, out, n):
        out.copy_(torch.where(x >= 0, g, g * slope))
        return 0


class _ConvFwdRounded(Emulator):
    def conv2d_fwd(self, x, w, bias, residual, y, B, Cin, Cout, H, W, ks):
        return super().conv2d_fwd(_round_mantissa(x), _round_mantissa(w), bias, residual, y, B, Cin, Cout, H, W, ks)


MUTANTS = {'bn_dbwd_a_gamma_x1.001': _ScaledAGamma, 'conv_dgrad_drops_last_cout': _DgradDropsLastChannel,
           'lrelu_derivative_at_zero_flipped': _LReluGeAtZero, 'conv_fwd_16_mantissa_bits': _ConvFwdRounded}


@pytest.mark.parametrize('name', sorted(MUTANTS))
def test_harness_rejects_a_wrong_emulator(name):
    backend._set_backend_for_testing(MUTANTS[name]())
    rejected = [c.name for c in CASES if SO.run_case(c, 'cpu')[1]]
    assert rejected, f'{name}: no case noticed'


def test_mantissa_rounding_is_an_accuracy_only_mutation():
    x = torch.randn(10000)
    rel = float(((_round_mantissa(x) - x) / x).abs().max())
    assert 1e-6 < rel <= 2 ** -17
