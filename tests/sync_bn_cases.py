"""Synchronised BatchNorm (tg_bn_sync_{stats,bwd,dbwd}_{local,finish}) against stock torch in float64 on the GLOBAL batch.

``SyncRanks`` plays W ranks in lockstep in one process, through the C ABI exactly as ``tartangan_amd.functional`` does
(``_BNAct``, ``_bn_bwd_into``, ``_BNActBwd``): every pass calls ``*_local`` on every shard, adds the W float64 sum vectors
(the SUM all-reduce), then calls ``*_finish`` on every shard with the total.  Each rank owns its shard, its mean / invstd /
running buffers / num_batches_tracked and its workspace.  No torch.distributed, no extra process: 8 ranks cost nothing.

The reference is ``F.leaky_relu(F.batch_norm(x, rm, rv, gamma, beta, True, momentum, eps), slope)`` on the global batch, its
first backward ``autograd.grad(<z, gz>, (x, gamma, beta))`` and its second backward (the gradients of <gx, v> with respect to
(gz, x, gamma), gx built under ``create_graph``), in float64 and in fp32 on the CPU.  The pass rule and every number in it are
those of tests/second_order_cases.py ("no worse than plain fp32"): ``errors`` / ``violations``.

What is compared, per case:
  fwd.*   mean, invstd (all ranks hold the same bits), running_mean, running_var (unbiased with n = replicate * W * B * HW),
          z (the shards' outputs, concatenated); num_batches_tracked += 1 exactly
  bwd.*   gx (concatenated), sum_r ggamma_r, sum_r gbeta_r; with ``variants``: accumulate = 1, gx = None, gx_add
  dbwd.*  adj_gz, adj_x (concatenated), sum_r adj_gamma_r (each rank's share is 1/W of the full-batch adjoint, and the shares of
          the W ranks are AVERAGED by the gradient all-reduce: W * mean_r = sum_r); with ``variants``: accumulate = 1
"""
import re

import torch
import torch.nn.functional as F

import second_order_cases as SO
from second_order_cases import MARGIN, _fix_bn, errors, violations

EPS_BN, MOMENTUM = 1e-5, 0.1
SYNC_ENTRY_POINTS = ('bn_sync_stats_local', 'bn_sync_stats_finish', 'bn_sync_bwd_local', 'bn_sync_bwd_finish',
                     'bn_sync_dbwd_local', 'bn_sync_dbwd_finish')
TG_EINVAL = -1
GLOBAL_ELEMENT_CAP = 2 ** 25          # W = 8 runs of the recorded layers: only those whose global tensor stays below this


class Spec:
    """One case: ``W`` ranks of ``(B, C, HW)`` each.  ``values``: how the global batch is drawn (see ``make_inputs``);
    ``unaligned``: every float tensor one float off a 16-byte boundary; ``variants``: also accumulate / gx = None / gx_add."""

    def __init__(self, name, W, B, C, HW, slope=0.2, replicate=1, values='shifted', unaligned=False, variants=True, blocks=None):
        self.name, self.W, self.B, self.C, self.HW = name, W, B, C, HW
        self.slope, self.replicate, self.values, self.unaligned, self.variants = slope, replicate, values, unaligned, variants
        self.blocks = blocks or W       # the number of image blocks with statistics of their own (rank-count invariance: fixed)

    def __repr__(self):
        return self.name


def _name(tag, W, B, C, HW, slope, replicate):
    return f'{tag}[W{W},{B}x{C}x{HW},s{slope},r{replicate}]'


# --------------------------------------------------------------------------- inputs
def make_inputs(spec, seed=0):
    """-> {x (W*B, C, HW, 1), gamma, beta, rm, rv, gz, v, gx_add, gg0, gb0, ag0}: fp32 CPU tensors of the GLOBAL batch."""
    gen = torch.Generator().manual_seed(seed)
    N, C, HW = spec.W * spec.B, spec.C, spec.HW
    rn = lambda *s: torch.randn(*s, generator=gen)
    gamma, beta = 1 + 0.3 * rn(C), 0.3 * rn(C)
    if spec.values in ('shifted', 'offset1e3'):
        # every block of images (a rank's shard, or a part of it) has its own scale and shift: shards with different statistics
        x = rn(N, C, HW, 1)
        k = spec.blocks
        scale = (0.5 + 1.5 * torch.arange(k) / max(k - 1, 1)).repeat_interleave(N // k).view(N, 1, 1, 1)
        shift = (0.8 * (torch.arange(k) - (k - 1) / 2)).repeat_interleave(N // k).view(N, 1, 1, 1)
        # (plus a common per-channel level: the statistics themselves are compared, and a global mean that cancels to ~0 would
        # measure the conditioning of that cancellation against the mean's own norm, not the arithmetic)
        x = x * scale + shift * (1 + 0.5 * rn(1, C, 1, 1)) + (1 + 0.5 * rn(1, C, 1, 1))
        if spec.values == 'offset1e3':
            x = 1e3 + 1e-2 * x                      # a large common offset: the pivot of sync_stats_pack
    elif spec.values == 'zero':
        # every channel of every shard balanced over {-1, 0, 1}, beta = 0: mean exactly 0, y exactly +-0 at a third of the elements
        n = spec.B * HW
        assert n % 3 == 0
        vals = torch.tensor([-1.0, 0.0, 1.0]).repeat_interleave(n // 3)
        shards = []
        for _ in range(spec.W):
            s = torch.stack([vals[torch.randperm(n, generator=gen)] for _ in range(C)], 0).view(C, spec.B, HW)
            s[s == 0] = torch.where(torch.rand(int((s == 0).sum()), generator=gen) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
            shards.append(s.transpose(0, 1))
        x = torch.cat(shards, 0).contiguous().view(N, C, HW, 1)
        beta = torch.zeros(C)
    elif spec.values == 'constant':
        # every other channel constant over ALL ranks (zero variance); beta off 0 there, so y keeps one sign in any arithmetic
        x = rn(N, C, HW, 1)
        x[:, ::2] = (0.1 + torch.rand(1, (C + 1) // 2, 1, 1, generator=gen)).expand(N, -1, HW, 1)
        beta = torch.where(beta.abs() < 0.05, torch.full_like(beta, 0.1), beta)
    elif spec.values == 'rank_constant':
        # constant within each rank, different between ranks: all variance is the between-rank term mean(mu_r^2) - mean(mu_r)^2
        x = rn(spec.W, 1, C, 1, 1).expand(spec.W, spec.B, C, HW, 1).reshape(N, C, HW, 1).contiguous()
    else:
        raise ValueError(spec.values)
    t = {'x': x, 'gamma': gamma, 'beta': beta}
    if spec.slope != 1 and spec.values in ('shifted', 'offset1e3', 'constant'):
        _fix_bn(t, gen)                             # (fails if it cannot finish in 100 rounds)
    if spec.values == 'rank_constant' and spec.slope != 1:
        xd = x.double()
        m, var = xd.mean((0, 2, 3), keepdim=True), xd.var((0, 2, 3), unbiased=False, keepdim=True)
        y = (xd - m) / torch.sqrt(var + EPS_BN) * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
        assert not (y.abs() < MARGIN).any(), 'rank-constant inputs on the LeakyReLU kink: pick another seed'
    t.update(rm=0.5 * rn(C), rv=0.5 + torch.rand(C, generator=gen), gz=rn(N, C, HW, 1), v=rn(N, C, HW, 1), gx_add=rn(N, C, HW, 1),
             gg0=rn(spec.W, C), gb0=rn(spec.W, C), ag0=rn(spec.W, C))
    return t


# --------------------------------------------------------------------------- the reference: stock torch on the global batch
def reference(spec, t, dtype):
    """-> {label: float64 CPU tensor} of every compared quantity, computed in ``dtype`` on the CPU."""
    c = lambda k: t[k].to(dtype)
    x, gamma, beta, gz = (c(k).clone().requires_grad_() for k in ('x', 'gamma', 'beta', 'gz'))
    rm, rv = c('rm').clone(), c('rv').clone()
    if spec.replicate == 1:
        y = F.batch_norm(x, rm, rv, gamma, beta, True, MOMENTUM, EPS_BN)
    else:
        # x stands for a tensor holding every element ``replicate`` times along the plane: the running statistics come from that
        F.batch_norm(x.detach().repeat_interleave(spec.replicate, 2), rm, rv, None, None, True, MOMENTUM, EPS_BN)
        y = F.batch_norm(x, None, None, gamma, beta, True, MOMENTUM, EPS_BN)
    z = F.leaky_relu(y, spec.slope)
    _, mean, invstd = torch.native_batch_norm(x.detach(), None, None, None, None, True, MOMENTUM, EPS_BN)
    out = {'fwd.mean': mean, 'fwd.invstd': invstd, 'fwd.running_mean': rm, 'fwd.running_var': rv, 'fwd.z': z}
    gx, gg, gb = torch.autograd.grad((z * gz).sum(), (x, gamma, beta), create_graph=True)
    out.update({'bwd.gx': gx, 'bwd.ggamma': gg, 'bwd.gbeta': gb})
    a_gz, a_x, a_gamma = torch.autograd.grad((gx * c('v')).sum(), (gz, x, gamma))
    out.update({'dbwd.adj_gz': a_gz, 'dbwd.adj_x': a_x, 'dbwd.adj_gamma': a_gamma})
    if spec.variants:
        out['bwd+acc.ggamma'] = gg + c('gg0').sum(0)
        out['bwd+acc.gbeta'] = gb + c('gb0').sum(0)
        out['bwd+add.gx'] = gx + c('gx_add')
        out['dbwd+acc.adj_gamma'] = a_gamma + c('ag0').sum(0)
    return {k: v.detach().to(torch.float64) for k, v in out.items()}


def references(spec, seed=0):
    t = make_inputs(spec, seed)
    return t, reference(spec, t, torch.float64), reference(spec, t, torch.float32)


# --------------------------------------------------------------------------- W ranks in lockstep through the C ABI
def call(K, name, *args):
    """The entry point's return code (the HIP binding raises on a non-zero code; the emulator returns it)."""
    from tartangan_amd.backend import KernelError
    try:
        return int(getattr(K, name)(*args) or 0)
    except KernelError as e:
        return int(re.search(r'code (-?\d+)', str(e)).group(1))


class SyncRanks:
    def __init__(self, K, device, spec, t, running=True, nbt=True):
        self.K, self.dev, self.spec = K, device, spec
        W, B, C, HW = spec.W, spec.B, spec.C, spec.HW
        self.dims = (B, C, HW)
        shard = lambda k: [self.put(t[k][r * B:(r + 1) * B]) for r in range(W)]
        self.x, self.gz, self.v, self.gx_add = shard('x'), shard('gz'), shard('v'), shard('gx_add')
        self.gamma, self.beta = self.put(t['gamma']), self.put(t['beta'])
        self.mean, self.invstd = [self.new(C) for _ in range(W)], [self.new(C) for _ in range(W)]
        self.rm = [self.put(t['rm']) if running else None for _ in range(W)]
        self.rv = [self.put(t['rv']) if running else None for _ in range(W)]
        self.nbt0 = 5
        self.nbt = [torch.full((), self.nbt0, dtype=torch.int64, device=device) if nbt else None for _ in range(W)]
        self.ws = [torch.empty(max(1, (int(K.bn_workspace(B, C, HW)) + 3) // 4), dtype=torch.float32, device=device) for _ in range(W)]

    # float tensors: optionally one float past a 16-byte boundary (a [1:] view of a larger buffer)
    def new(self, *shape):
        n = 1
        for s in shape:
            n *= s
        if self.spec.unaligned:
            return torch.empty(n + 1, dtype=torch.float32, device=self.dev)[1:].view(*shape)
        return torch.empty(*shape, dtype=torch.float32, device=self.dev)

    def put(self, src):
        out = self.new(*src.shape)
        out.copy_(src)
        return out

    def _sums(self, k):
        return [torch.empty(self.spec.C * k, dtype=torch.float64, device=self.dev) for _ in range(self.spec.W)]

    def _all_reduce(self, sums):
        total = sums[0].clone()
        for s in sums[1:]:
            total += s
        return total

    def _cat(self, parts):
        return torch.cat([p.detach().to('cpu', torch.float64) for p in parts], 0)

    def _sum(self, parts):
        return torch.stack(parts, 0).sum(0).to('cpu', torch.float64)

    def forward(self):
        K, sp, (B, C, HW) = self.K, self.spec, self.dims
        sums = self._sums(3)
        for r in range(sp.W):
            assert call(K, 'bn_sync_stats_local', self.x[r], sums[r], self.ws[r], B, C, HW) == 0
        total = self._all_reduce(sums)
        z = [self.new(B, C, HW, 1) for _ in range(sp.W)]
        for r in range(sp.W):
            assert call(K, 'bn_sync_stats_finish', total.clone(), sp.W, self.mean[r], self.invstd[r], self.rm[r], self.rv[r],
                        self.nbt[r], MOMENTUM, EPS_BN, sp.W * B * HW, sp.replicate, C) == 0
            assert call(K, 'bn_act_fwd', self.x[r], self.mean[r], self.invstd[r], self.gamma, self.beta, float(sp.slope), z[r], B, C, HW) == 0
        for r in range(1, sp.W):
            assert torch.equal(self.mean[r], self.mean[0]) and torch.equal(self.invstd[r], self.invstd[0]), 'ranks disagree on the statistics'
            if self.rm[0] is not None:
                assert torch.equal(self.rm[r], self.rm[0]) and torch.equal(self.rv[r], self.rv[0]), 'ranks disagree on the running statistics'
        for n in self.nbt:
            if n is not None:
                assert int(n) == self.nbt0 + 1, f'num_batches_tracked {int(n)} after one call from {self.nbt0}'
        self.nbt0 += 1
        out = {'fwd.mean': self.mean[0].to('cpu', torch.float64), 'fwd.invstd': self.invstd[0].to('cpu', torch.float64), 'fwd.z': self._cat(z)}
        if self.rm[0] is not None:
            out.update({'fwd.running_mean': self.rm[0].to('cpu', torch.float64), 'fwd.running_var': self.rv[0].to('cpu', torch.float64)})
        return out

    def backward(self, tag='bwd', accumulate=0, want_gx=True, gx_add=False, init=None):
        """-> {tag.gx, tag.ggamma, tag.gbeta}; ``init``: (gg0, gb0) per rank, the contents accumulate = 1 adds onto."""
        K, sp, (B, C, HW) = self.K, self.spec, self.dims
        local = self._sums(2)
        for r in range(sp.W):
            assert call(K, 'bn_sync_bwd_local', self.gz[r], self.x[r], self.mean[r], self.invstd[r], self.gamma, self.beta, float(sp.slope),
                        local[r], self.ws[r], B, C, HW) == 0
        total = self._all_reduce(local)
        gx = [self.new(B, C, HW, 1) if want_gx else None for _ in range(sp.W)]
        gg = [self.put(init[0][r]) if init else self.new(C) for r in range(sp.W)]
        gb = [self.put(init[1][r]) if init else self.new(C) for r in range(sp.W)]
        for r in range(sp.W):
            assert call(K, 'bn_sync_bwd_finish', self.gz[r], self.x[r], self.mean[r], self.invstd[r], self.gamma, self.beta, float(sp.slope),
                        local[r], total.clone(), sp.W * B * HW, gx[r], gg[r], gb[r], self.ws[r], B, C, HW, accumulate,
                        self.gx_add[r] if gx_add else None) == 0
        out = {f'{tag}.ggamma': self._sum(gg), f'{tag}.gbeta': self._sum(gb)}
        if want_gx:
            out[f'{tag}.gx'] = self._cat(gx)
        return out

    def second_backward(self, tag='dbwd', accumulate=0, init=None):
        K, sp, (B, C, HW) = self.K, self.spec, self.dims
        sums = self._sums(5)
        for r in range(sp.W):
            assert call(K, 'bn_sync_dbwd_local', self.v[r], self.gz[r], self.x[r], self.mean[r], self.invstd[r], self.gamma, self.beta,
                        float(sp.slope), sums[r], self.ws[r], B, C, HW) == 0
        total = self._all_reduce(sums)
        a_gz, a_x = [self.new(B, C, HW, 1) for _ in range(sp.W)], [self.new(B, C, HW, 1) for _ in range(sp.W)]
        a_gamma = [self.put(init[r]) if init is not None else self.new(C) for r in range(sp.W)]
        for r in range(sp.W):
            assert call(K, 'bn_sync_dbwd_finish', self.v[r], self.gz[r], self.x[r], self.mean[r], self.invstd[r], self.gamma, self.beta,
                        float(sp.slope), total.clone(), sp.W * B * HW, sp.W, a_gz[r], a_x[r], a_gamma[r], self.ws[r], B, C, HW, accumulate) == 0
        return {f'{tag}.adj_gz': self._cat(a_gz), f'{tag}.adj_x': self._cat(a_x), f'{tag}.adj_gamma': self._sum(a_gamma)}


def run_sync(K, device, spec, t):
    """Every compared quantity of ``reference`` from the W-rank protocol on backend ``K``."""
    ranks = SyncRanks(K, device, spec, t)
    out = ranks.forward()
    out.update(ranks.backward())
    out.update(ranks.second_backward())
    if spec.variants:
        acc = ranks.backward('bwd+acc', accumulate=1, init=(t['gg0'], t['gb0']))
        out.update({k: acc[k] for k in ('bwd+acc.ggamma', 'bwd+acc.gbeta')})
        # gx = None: the parameter gradients are those of the call that also writes gx
        nogx = ranks.backward('bwd-gx', want_gx=False)
        assert torch.equal(nogx['bwd-gx.ggamma'], out['bwd.ggamma']) and torch.equal(nogx['bwd-gx.gbeta'], out['bwd.gbeta']), \
            'gx = None changed the parameter gradients'
        add = ranks.backward('bwd+add', gx_add=True)
        assert torch.equal(add['bwd+add.ggamma'], out['bwd.ggamma']) and torch.equal(add['bwd+add.gbeta'], out['bwd.gbeta'])
        out['bwd+add.gx'] = add['bwd+add.gx']
        out['dbwd+acc.adj_gamma'] = ranks.second_backward('dbwd+acc', accumulate=1, init=t['ag0'])['dbwd+acc.adj_gamma']
    return out


def run_local(K, device, spec, t):
    """The local-statistics kernels (bn_train_fwd / bn_act_bwd / bn_act_dbwd) on the same data: W must be 1."""
    assert spec.W == 1
    rk = SyncRanks(K, device, spec, t)
    (B, C, HW), r = rk.dims, 0
    z, gx, gg, gb = rk.new(B, C, HW, 1), rk.new(B, C, HW, 1), rk.new(C), rk.new(C)
    a_gz, a_x, a_gamma = rk.new(B, C, HW, 1), rk.new(B, C, HW, 1), rk.new(C)
    assert call(K, 'bn_train_fwd', rk.x[r], rk.mean[r], rk.invstd[r], rk.rm[r], rk.rv[r], rk.nbt[r], rk.gamma, rk.beta, float(spec.slope),
                MOMENTUM, EPS_BN, z, rk.ws[r], B, C, HW, spec.replicate) == 0
    assert call(K, 'bn_act_bwd', rk.gz[r], rk.x[r], rk.mean[r], rk.invstd[r], rk.gamma, rk.beta, float(spec.slope), 1, gx, gg, gb, rk.ws[r],
                B, C, HW, 0, None) == 0
    assert call(K, 'bn_act_dbwd', rk.v[r], None, None, rk.gz[r], rk.x[r], rk.mean[r], rk.invstd[r], rk.gamma, rk.beta, float(spec.slope),
                a_gz, a_x, a_gamma, rk.ws[r], B, C, HW, 0) == 0
    assert int(rk.nbt[r]) == rk.nbt0 + 1
    out = {'fwd.mean': rk.mean[r], 'fwd.invstd': rk.invstd[r], 'fwd.running_mean': rk.rm[r], 'fwd.running_var': rk.rv[r], 'fwd.z': z,
           'bwd.gx': gx, 'bwd.ggamma': gg, 'bwd.gbeta': gb, 'dbwd.adj_gz': a_gz, 'dbwd.adj_x': a_x, 'dbwd.adj_gamma': a_gamma}
    return {k: v.detach().to('cpu', torch.float64) for k, v in out.items()}


def check(spec, got, r64, r32):
    """-> (errors, violations) under the rule of second_order_cases."""
    assert set(got) == set(r64), sorted(set(got) ^ set(r64))
    errs = errors(got, r64, r32)
    return errs, [f'{spec.name} {b}' for b in violations(errs)]


def run_case(K, device, spec, refs=None, seed=0):
    t, r64, r32 = refs if refs is not None else references(spec, seed)
    return check(spec, run_sync(K, device, spec, t), r64, r32)


def worst_ratios(errs):
    """{pass: worst e_op / max(e_32, EPS)} -- what the rule bounds by RATIO_L2."""
    worst = {}
    for k, (e, e32, *_rest) in errs.items():
        p = k.split('.')[0].split('+')[0].split('-')[0]
        worst[p] = max(worst.get(p, 0.0), e / max(e32, SO.EPS))
    return worst


def report(spec, errs, tag='SYNCBN'):
    print(f'{tag} {spec.name} ' + ' '.join(f'{k}={v:.2f}' for k, v in sorted(worst_ratios(errs).items())))


# --------------------------------------------------------------------------- nullable forms, rejection, replicate
def check_nullable_and_rejected_forms(K, device, spec, t, r64, r32):
    """rm = rv = None and nbt = None run and leave the same statistics; one of rm / rv alone is rejected with TG_EINVAL and
    touches nothing.  -> violations."""
    full = SyncRanks(K, device, spec, t).forward()
    bare = SyncRanks(K, device, spec, t, running=False, nbt=False).forward()
    assert set(bare) == {'fwd.mean', 'fwd.invstd', 'fwd.z'}
    for k in bare:
        assert torch.equal(bare[k], full[k]), k
    no_nbt = SyncRanks(K, device, spec, t, nbt=False).forward()
    for k in full:
        assert torch.equal(no_nbt[k], full[k]), k
    rk = SyncRanks(K, device, spec, t)
    B, C, HW = rk.dims
    sums = rk._sums(3)
    assert call(K, 'bn_sync_stats_local', rk.x[0], sums[0], rk.ws[0], B, C, HW) == 0
    for rm, rv in ((rk.rm[0], None), (None, rk.rv[0])):
        rc = call(K, 'bn_sync_stats_finish', sums[0], 1, rk.mean[0], rk.invstd[0], rm, rv, rk.nbt[0], MOMENTUM, EPS_BN, B * HW, 1, C)
        assert rc == TG_EINVAL, rc
    assert int(rk.nbt[0]) == rk.nbt0 and torch.equal(rk.rm[0].cpu(), t['rm']) and torch.equal(rk.rv[0].cpu(), t['rv'])
    return check(spec, {k: full[k] for k in full}, {k: r64[k] for k in full}, {k: r32[k] for k in full})[1]


def check_replicate_only_moves_running_var(K, device, spec, t):
    """The same data with replicate = 1 and replicate = 4: only running_var may differ, and it does."""
    assert spec.replicate > 1
    one = Spec(spec.name, spec.W, spec.B, spec.C, spec.HW, spec.slope, 1, spec.values, spec.unaligned, False, spec.blocks)
    a, b = SyncRanks(K, device, one, t).forward(), SyncRanks(K, device, spec, t).forward()
    for k in a:
        if k != 'fwd.running_var':
            assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a['fwd.running_var'], b['fwd.running_var'])
    assert not torch.equal(reference(one, t, torch.float64)['fwd.running_var'], reference(spec, t, torch.float64)['fwd.running_var'])


# --------------------------------------------------------------------------- exact edges
def check_zero_edge(K, device, spec, refs):
    """Pre-activations of exactly +0.0 and -0.0 (every shard balanced over {-1, +-0, 1}, beta = 0: the mean is exactly 0 in any
    arithmetic).  z is exactly 0 there, and the first- and second-backward masks give ``slope`` like torch: a mask of 1 there
    puts an O(1) error on a third of gx and adj_gz."""
    t, r64, r32 = refs
    got = run_sync(K, device, spec, t)
    at_zero = (t['x'] == 0).double()
    assert float(at_zero.mean()) > 0.3 and bool((t['x'][t['x'] == 0].view(torch.int32) != 0).any())      # both +0.0 and -0.0
    assert torch.equal(got['fwd.mean'], torch.zeros(spec.C, dtype=torch.float64))
    assert torch.equal(got['fwd.z'] * at_zero, torch.zeros_like(at_zero)) and torch.equal(r32['fwd.z'] * at_zero, torch.zeros_like(at_zero))
    errs, bad = check(spec, got, r64, r32)
    assert not bad, bad
    return errs


def check_constant_edge(K, device, spec, refs):
    """Every other channel constant over all ranks: mean == the constant, invstd == 1/sqrt(eps) rounded once (eps as the float
    the C ABI receives), exactly; z, gx and adj_x finite and within the rule of torch's."""
    t, r64, r32 = refs
    got = run_sync(K, device, spec, t)
    n_const = (spec.C + 1) // 2
    eps32 = float(torch.tensor(EPS_BN, dtype=torch.float32))
    once = torch.tensor(1.0 / eps32 ** 0.5, dtype=torch.float64).float().double()
    assert torch.equal(got['fwd.invstd'][::2], once.expand(n_const)), (got['fwd.invstd'][::2], once)
    assert torch.equal(got['fwd.mean'][::2], t['x'][0, ::2, 0, 0].double())
    for k in ('fwd.z', 'bwd.gx', 'dbwd.adj_x', 'dbwd.adj_gz'):
        assert bool(torch.isfinite(got[k]).all()), k
    # (z there is lrelu(beta) in exact arithmetic only: the kernels' fma(x, gamma r, beta - mean gamma r) and torch's own fp32
    # mean both leave ~ulp(x gamma r) on it, so z, gx and adj_x are held to the rule)
    errs, bad = check(spec, got, r64, r32)
    assert not bad, bad
    return errs


# --------------------------------------------------------------------------- the case tables
EDGE_SHAPES = [(4, 3, 30 * 30), (2, 7, 12 * 10), (8, 128, 1), (5, 100, 8 * 8), (3, 130, 16 * 16), (2, 16, 128 * 128)]


def edge_shape_specs():
    """C < 8, C % 64 != 0, both sides of small_case(), HW = 1; slope in {0.2, 1}, replicate in {1, 4}, W in {2, 4, 8}."""
    out = []
    for i, (B, C, HW) in enumerate(EDGE_SHAPES):
        for j, (slope, rep) in enumerate(((0.2, 1), (1.0, 4), (0.2, 4), (1.0, 1))):
            W = (2, 4, 8)[(i + j) % 3]
            out.append(Spec(_name('edge', W, B, C, HW, slope, rep), W, B, C, HW, slope, rep))
    return out


def offset_specs():
    return [Spec(_name('offset1e3', W, B, C, HW, 0.2, rep), W, B, C, HW, 0.2, rep, values='offset1e3')
            for W, (B, C, HW), rep in ((2, EDGE_SHAPES[0], 1), (4, EDGE_SHAPES[3], 4), (8, EDGE_SHAPES[4], 1))]


def unaligned_specs():
    """Every float tensor one float off a 16-byte boundary: the reduce and the map take their scalar paths (both plane sizes)."""
    return [Spec(_name('unaligned', 2, B, C, HW, 0.2, 1), 2, B, C, HW, 0.2, 1, unaligned=True)
            for B, C, HW in (EDGE_SHAPES[4], EDGE_SHAPES[5])]


INVARIANCE_GLOBAL = [(16, 24, 12 * 12), (8, 70, 32 * 32)]
INVARIANCE_WORLDS = (1, 2, 4, 8)


def invariance_specs():
    """One global batch (8 blocks of images with statistics of their own) split over 1, 2, 4 and 8 ranks."""
    return {(N, C, HW): [Spec(_name('split', W, N // W, C, HW, 0.2, 1), W, N // W, C, HW, 0.2, 1, variants=False, blocks=8)
                         for W in INVARIANCE_WORLDS] for N, C, HW in INVARIANCE_GLOBAL}


def zero_specs():
    return [Spec(_name('zero', W, 3, 5, 99, slope, 1), W, 3, 5, 99, slope, 1, values='zero', variants=False) for W, slope in ((2, 0.2), (4, 0.0))]


def constant_specs():
    return [Spec(_name('constant', W, 3, 6, 99, 0.2, 1), W, 3, 6, 99, 0.2, 1, values='constant', variants=False) for W in (2, 8)]


def rank_constant_specs():
    return [Spec(_name('rank_constant', W, 3, 6, 99, 0.2, 1), W, 3, 6, 99, 0.2, 1, values='rank_constant', variants=False) for W in (2, 8)]


def small_specs():
    """Everything but the recorded layers: cheap enough to run on every backend, and what the wrong variants are tried on."""
    inv = [s for group in invariance_specs().values() for s in group]
    return edge_shape_specs() + offset_specs() + unaligned_specs() + inv + zero_specs() + constant_specs() + rank_constant_specs()


# --------------------------------------------------------------------------- the networks' own BatchNorm layers
RECORD_CONFIG, RECORD_BATCH = '128:3', 32


def record_bn_layers(K, device):
    """{(B, C, HW, replicate)} of every BatchNorm of the 128:3 generator and discriminator, from the launches of one
    local-statistics training step at batch 32 (the grouped real | fake launch is one layer per group of B images)."""
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    from tartangan_amd.trainers.cnn import CNNTrainer
    name, att = RECORD_CONFIG.split(':')
    cfg = GAN_CONFIGS[name]._replace(attention=(int(att),))
    tr = CNNTrainer(CNNTrainer.default_args(config=cfg, batch_size=RECORD_BATCH, device=device))
    torch.manual_seed(1234)
    tr.build_models()
    g = torch.Generator().manual_seed(7)
    size = int(name)
    with SO.Recorder(K, ('bn_train_fwd', 'bn_train_fwd_groups')) as rec:
        tr.train_batch((torch.rand(RECORD_BATCH, 3, size, size, generator=g) * 2 - 1).to(device))
    layers = {(B, C, HW, rep) for B, C, HW, rep in rec.seen.get('bn_train_fwd', ())}
    layers |= {(B, C, HW, rep) for G, B, C, HW, rep in rec.seen.get('bn_train_fwd_groups', ())}
    assert layers and all(B == RECORD_BATCH for B, *_ in layers), sorted(layers)
    return layers


def layer_specs(layers):
    """-> (W = 2 specs of every recorded layer, W = 8 specs of those below the element cap); asserts the dropped share."""
    layers = sorted(layers)
    two = [Spec(_name('layer', 2, B, C, HW, 0.2, rep), 2, B, C, HW, 0.2, rep, variants=False) for B, C, HW, rep in layers]
    kept = [(B, C, HW, rep) for B, C, HW, rep in layers if 8 * B * C * HW < GLOBAL_ELEMENT_CAP]
    assert 3 * (len(layers) - len(kept)) <= len(layers), (len(layers), len(kept))
    eight = [Spec(_name('layer', 8, B, C, HW, 0.2, rep), 8, B, C, HW, 0.2, rep, variants=False) for B, C, HW, rep in kept]
    return two, eight
