"""The SyncBN cases (tests/sync_bn_cases.py) on the emulator: the W-rank protocol of tests/emulator.py -- which the HIP kernels
are held to in tests/test_sync_bn_gpu.py -- against stock torch on the global batch in float64.  It is also the evidence that
the references and the inputs themselves stay inside the caps (every case draws its inputs off the LeakyReLU kink).  Then proof
that the cases have teeth: seven one-line wrong variants of the protocol must each be rejected."""
import pytest
import torch

import sync_bn_cases as SB
from emulator import Emulator

SMALL = SB.small_specs()
_REFS = {}


def _refs(spec):
    if spec.name not in _REFS:
        _REFS[spec.name] = SB.references(spec)
    return _REFS[spec.name]


@pytest.mark.parametrize('spec', SB.edge_shape_specs() + SB.offset_specs() + SB.unaligned_specs(), ids=repr)
def test_sync_passes_match_float64_torch_on_the_global_batch(spec):
    errs, bad = SB.run_case(Emulator(), 'cpu', spec, _refs(spec))
    assert not bad, bad
    assert {'fwd.running_var', 'bwd.ggamma', 'bwd+acc.gbeta', 'bwd+add.gx', 'dbwd.adj_gamma', 'dbwd+acc.adj_gamma', 'dbwd.adj_x'} <= set(errs)


def test_case_table_covers_the_shapes_and_values_asked_for():
    specs = SB.edge_shape_specs()
    assert {(s.B, s.C, s.HW) for s in specs} == set(SB.EDGE_SHAPES)
    assert {s.slope for s in specs} == {0.2, 1.0} and {s.replicate for s in specs} == {1, 4} and {s.W for s in specs} == {2, 4, 8}
    assert any(s.C < 8 for s in specs) and any(s.C % 64 for s in specs) and any(s.HW == 1 for s in specs)
    assert {s.W for group in SB.invariance_specs().values() for s in group} == {1, 2, 4, 8}
    # shards with different statistics: the local means of a case differ by more than the channel's standard deviation / 4
    t = SB.make_inputs(specs[0])
    means = t['x'].view(specs[0].W, specs[0].B, specs[0].C, -1).mean((1, 3))
    assert float((means.max(0).values - means.min(0).values).min()) > 0.25 * float(t['x'].std())
    # the unaligned run really is off a 16-byte boundary, every float tensor of it
    rk = SB.SyncRanks(Emulator(), 'cpu', SB.unaligned_specs()[0], SB.make_inputs(SB.unaligned_specs()[0]))
    for ten in rk.x + rk.gz + rk.v + rk.gx_add + rk.mean + rk.invstd + rk.rm + rk.rv + [rk.gamma, rk.beta, rk.new(4, 4)]:
        assert ten.data_ptr() % 16 == 4 and ten.is_contiguous()


@pytest.mark.parametrize('shape', sorted(SB.invariance_specs()), ids=str)
def test_rank_count_invariance(shape):
    """One global batch over 1, 2, 4 and 8 ranks: every split within the rule (of the SAME references), and W = 1 next to the
    local-statistics kernels on the same data."""
    group = SB.invariance_specs()[shape]
    t, r64, r32 = SB.references(group[0])
    for spec in group:
        assert torch.equal(SB.make_inputs(spec)['x'], t['x'])
        errs, bad = SB.check(spec, SB.run_sync(Emulator(), 'cpu', spec, t), r64, r32)
        assert not bad, bad
    errs, bad = SB.check(group[0], SB.run_local(Emulator(), 'cpu', group[0], t), r64, r32)
    assert not bad, bad


@pytest.mark.parametrize('spec', [SB.edge_shape_specs()[0], SB.edge_shape_specs()[9]], ids=repr)
def test_nullable_buffers_and_rejected_forms(spec):
    t, r64, r32 = _refs(spec)
    bad = SB.check_nullable_and_rejected_forms(Emulator(), 'cpu', spec, t, r64, r32)
    assert not bad, bad


@pytest.mark.parametrize('spec', [s for s in SB.edge_shape_specs() if s.replicate == 4][:4], ids=repr)
def test_replicate_moves_running_var_and_nothing_else(spec):
    SB.check_replicate_only_moves_running_var(Emulator(), 'cpu', spec, _refs(spec)[0])


def test_network_layers_at_two_and_eight_ranks():
    """Every BatchNorm of the 128:3 generator and discriminator (recorded from one local-statistics step at batch 32) as 2 ranks
    of 32, and as 8 ranks of 32 where the global tensor stays below 2^25 elements: every case draws its inputs off the kink and
    the emulated protocol stays within the rule."""
    from tartangan_amd import backend
    K = Emulator()
    prev = backend._set_backend_for_testing(K)
    try:
        layers = SB.record_bn_layers(K, 'cpu')
    finally:
        backend._set_backend_for_testing(prev)
    two, eight = SB.layer_specs(layers)
    assert len(two) >= 10 and any(s.replicate == 4 for s in two) and 3 * len(eight) >= 2 * len(two)
    failures = []
    for spec in two + eight:
        refs = SB.references(spec)
        failures += SB.run_case(K, 'cpu', spec, refs)[1]
        del refs
    assert not failures, failures


# --------------------------------------------------------------------------- exact edges
@pytest.mark.parametrize('spec', SB.zero_specs(), ids=repr)
def test_lrelu_mask_at_exactly_zero_is_torchs(spec):
    SB.check_zero_edge(Emulator(), 'cpu', spec, _refs(spec))


@pytest.mark.parametrize('spec', SB.constant_specs(), ids=repr)
def test_channel_constant_over_all_ranks(spec):
    SB.check_constant_edge(Emulator(), 'cpu', spec, _refs(spec))


@pytest.mark.parametrize('spec', SB.rank_constant_specs(), ids=repr)
def test_channel_constant_within_each_rank(spec):
    errs, bad = SB.run_case(Emulator(), 'cpu', spec, _refs(spec))
    assert not bad, bad
    t = _refs(spec)[0]
    assert float(t['x'].view(spec.W, -1, spec.C, spec.HW).var(3).max()) == 0.0        # all variance is between ranks


# --------------------------------------------------------------------------- the cases have teeth
class _AdjGammaWithoutWorld(Emulator):
    def bn_sync_dbwd_finish(self, v, gz, x, mean, invstd, gamma, beta, slope, glob, count_global, world, *rest):
        return super().bn_sync_dbwd_finish(v, gz, x, mean, invstd, gamma, beta, slope, glob, count_global, 1, *rest)


class _ParamGradsFromGlobalSums(Emulator):
    def bn_sync_bwd_finish(self, gz, x, mean, invstd, gamma, beta, slope, local, glob, *rest):
        return super().bn_sync_bwd_finish(gz, x, mean, invstd, gamma, beta, slope, glob, glob, *rest)


class _CoefficientsOverLocalCount(Emulator):
    def bn_sync_bwd_finish(self, gz, x, mean, invstd, gamma, beta, slope, local, glob, count_global, gx, gg, gb, ws, B, C, HW, *rest):
        return super().bn_sync_bwd_finish(gz, x, mean, invstd, gamma, beta, slope, local, glob, B * HW, gx, gg, gb, ws, B, C, HW, *rest)

    def bn_sync_dbwd_finish(self, v, gz, x, mean, invstd, gamma, beta, slope, glob, count_global, world, a_gz, a_x, a_gamma, ws, B, C, HW,
                            *rest):
        return super().bn_sync_dbwd_finish(v, gz, x, mean, invstd, gamma, beta, slope, glob, B * HW, world, a_gz, a_x, a_gamma, ws,
                                           B, C, HW, *rest)


class _RunningVarCountWithoutReplicate(Emulator):
    def bn_sync_stats_finish(self, sums, world, mean, invstd, rm, rv, nbt, momentum, eps, count_global, replicate, C):
        return super().bn_sync_stats_finish(sums, world, mean, invstd, rm, rv, nbt, momentum, eps, count_global, 1, C)


class _VarianceWithoutBetweenRankTerm(Emulator):
    def bn_sync_stats_finish(self, sums, world, *rest):
        s = sums.view(-1, 3).clone()
        s[:, 1] = (s[:, 0] / world) ** 2 * world          # mean(mu_r^2) := mean(mu_r)^2
        return super().bn_sync_stats_finish(s.view(-1), world, *rest)


class _NbtPlusWorld(Emulator):
    def bn_sync_stats_finish(self, sums, world, mean, invstd, rm, rv, nbt, *rest):
        rc = super().bn_sync_stats_finish(sums, world, mean, invstd, rm, rv, nbt, *rest)
        if nbt is not None and rc == 0:
            nbt.add_(world - 1)
        return rc


class _MaskGreaterEqual(Emulator):
    @staticmethod
    def _bn_parts(x, mean, invstd, gamma, beta, slope, B, C, HW):
        xhat, y, _ = Emulator._bn_parts(x, mean, invstd, gamma, beta, slope, B, C, HW)
        return xhat, y, torch.where(y >= 0, torch.ones_like(y), torch.full_like(y, slope))


# variant -> (class, a case that must reject it)
MUTANTS = {
    'adj_gamma_without_/world': (_AdjGammaWithoutWorld, 'edge[W2,4x3x900,s0.2,r1]'),
    'ggamma_gbeta_from_global_sums': (_ParamGradsFromGlobalSums, 'edge[W2,4x3x900,s0.2,r1]'),
    'coefficients_over_local_count': (_CoefficientsOverLocalCount, 'edge[W2,4x3x900,s0.2,r1]'),
    'running_var_count_without_replicate': (_RunningVarCountWithoutReplicate, 'edge[W4,8x128x1,s0.2,r4]'),
    'variance_without_between_rank_term': (_VarianceWithoutBetweenRankTerm, 'rank_constant[W2,3x6x99,s0.2,r1]'),
    'nbt_plus_world': (_NbtPlusWorld, 'edge[W2,4x3x900,s0.2,r1]'),
    'lrelu_mask_greater_equal': (_MaskGreaterEqual, 'zero[W2,3x5x99,s0.2,r1]'),
}


def _rejects(K, spec):
    """Does the case fail on backend ``K``?  (A violation of the rule, or one of the driver's own exact assertions.)"""
    try:
        if spec.values == 'zero':
            SB.check_zero_edge(K, 'cpu', spec, _refs(spec))
            return False
        return bool(SB.run_case(K, 'cpu', spec, _refs(spec))[1])
    except AssertionError:
        return True


def test_the_unchanged_emulator_passes_every_small_case():
    assert [s.name for s in SMALL if _rejects(Emulator(), s)] == []


@pytest.mark.parametrize('name', sorted(MUTANTS))
def test_cases_reject_a_wrong_protocol(name):
    cls, expected = MUTANTS[name]
    rejected = [s.name for s in SMALL if _rejects(cls(), s)]
    print(f'SYNCBN_MUTANT {name}: rejected by {len(rejected)} of {len(SMALL)} cases, among them {expected}')
    assert expected in rejected, f'{name}: expected {expected} to reject it; rejected by {rejected or "no case"}'
