"""Checking kernels on tensors that cross 2 GiB, 4 GiB and 2^31 elements.  TEST INFRASTRUCTURE ONLY.

``guarded.run_both`` builds every tensor on the CPU and runs the emulator on all of it; at these extents neither is possible.
Instead:

  * PERIODIC inputs.  A base of ``P = 7`` images (planes, rows, blocks) comes from a seeded CPU generator and is tiled along
    the leading dimension ON THE DEVICE: ``x[b] = base[b % 7]``.  The reference is plain float64 torch on the CPU over the 7
    base images; the expected output of a per-image operation is that reference, tiled.  ``max_err`` compares every output
    element with it on the device, a chunk at a time (at most ``CHUNK`` elements as float64: 512 MiB), by max-abs difference;
    a NaN or an infinity anywhere makes the result non-finite.  Only scalars cross to the host.
  * Why 7: a wrapped 32-bit offset moves an access by 2^29, 2^30, 2^31 or 2^32 elements (``SHIFTS``).  With power-of-two
    images that is a power-of-two number of images, never a multiple of 7, so the wrapped access lands on other data.
    ``check_period`` asserts exactly that, before anything is allocated: no shift is a multiple of ``7 x per_image`` and, for
    image sizes that are no power of two, no shift is a whole number of images at all.
  * PROBES for reductions over the batch.  Inputs are integers in {-2..2}; the reduced operand is zero except at the probe
    images: the first, the last, and the two images either side of each 2^29, 2^30 and 2^31-element offset of every operand
    (``probes``).  ``check_exact`` asserts that the sum of the magnitudes of all terms stays below 2^24, so every partial
    sum is an integer fp32 holds exactly, in any summation order: the result must EQUAL the int64 reference.

Everything takes its boundaries as arguments, so tests/test_large_extents.py runs the same code on the CPU with the
boundaries scaled down to 2^12 elements, against the emulator and against deliberately defective emulators.
"""
import torch

P = 7
SHIFTS = (1 << 29, 1 << 30, 1 << 31, 1 << 32)        # elements a wrapped 32-bit element or byte offset moves an access by
OFFSETS = (1 << 29, 1 << 30, 1 << 31)                # element offsets whose neighbouring images are probes
CHUNK = 1 << 26                                      # elements per comparison chunk (512 MiB as float64)
EXACT = 1 << 24                                      # integers below this magnitude are exact in fp32
GIB = 1 << 30
MAX_NEED = 40 * GIB


# ---------------------------------------------------------------------------------------------- arithmetic, no allocation
def check_period(per_image, shifts=SHIFTS, period=P):
    """A wrapped access must land on different data: no shift may be a multiple of period x per_image elements, and where
    per_image is no power of two the shift must not be a whole number of images either (its sub-image remainder is nonzero)."""
    assert per_image > 0
    pow2 = per_image & (per_image - 1) == 0
    for s in shifts:
        assert s % (period * per_image) != 0, f'shift {s} is a multiple of {period} x {per_image}: periodic data cannot see it'
        if not pow2:
            assert s % per_image != 0, f'shift {s} is a whole number of {per_image}-element images'


def check_exact(n_terms, max_abs_term, bound=EXACT):
    """Every partial sum of n_terms terms of magnitude <= max_abs_term is an integer below 2^24: exact in fp32 in any order."""
    assert n_terms * max_abs_term < bound, f'{n_terms} terms of magnitude {max_abs_term} can reach {n_terms * max_abs_term} >= {bound}'


def probes(count, per_image_sizes, offsets=OFFSETS):
    """Images (of `count`) that a reduction's sparse operand is nonzero at: the first, the last, and for every operand
    (elements per image in per_image_sizes) the image holding each boundary element and the one before it."""
    out = {0, count - 1}
    for per in per_image_sizes:
        for off in offsets:
            for b in (off // per - 1, off // per):
                if 0 <= b < count:
                    out.add(b)
    return sorted(out)


def probe_counts(probe_list, period=P):
    """How many probes fall on each residue: the reduction's reference is sum_r counts[r] * term(base[r])."""
    counts = [0] * period
    for b in probe_list:
        counts[b % period] += 1
    return counts


# ---------------------------------------------------------------------------------------------- data
def base(*tail, seed=0, integer=False, nonzero=False, scale=1.0, period=P):
    """(period, *tail) float32 on the CPU: normal, or integers in {-2..2} ({-2,-1,1,2} with nonzero)."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * len(tail) + sum(tail))
    if not integer:
        return torch.randn(period, *tail, generator=g) * scale
    if nonzero:
        v = torch.randint(0, 4, (period, *tail), generator=g)
        return (v - 2 + (v >= 2).long()).float()
    return torch.randint(-2, 3, (period, *tail), generator=g).float()


def tile_flat(base_flat, n, device, step=1 << 28):
    """n elements on `device`, out[i] = base_flat[i % len(base_flat)], written a piece at a time (nothing of size n besides out)."""
    src = base_flat.reshape(-1).to(device)
    q = src.numel()
    out = torch.empty(n, dtype=src.dtype, device=device)
    per = max(1, step // q) * q
    for i0 in range(0, n, per):
        i1 = min(n, i0 + per)
        full = (i1 - i0) // q
        if full:
            out[i0:i0 + full * q].view(full, q).copy_(src.unsqueeze(0).expand(full, q))
        if i0 + full * q < i1:
            out[i0 + full * q:i1].copy_(src[:i1 - i0 - full * q])
    return out


def tile(base_t, count, device):
    """(count, *tail) on `device` with x[b] = base_t[b % P]."""
    per = base_t[0].numel()
    return tile_flat(base_t, count * per, device).view(count, *base_t.shape[1:])


def sparse(base_t, count, probe_list, device):
    """(count, *tail) of zeros with x[b] = base_t[b % P] at the probe images."""
    out = torch.zeros(count, *base_t.shape[1:], dtype=base_t.dtype, device=device)
    src = base_t.to(device)
    for b in probe_list:
        out[b].copy_(src[b % base_t.shape[0]])
    return out


def fresh(*shape, device, dtype=torch.float32):
    """An output nobody has written: NaN (0xA5 bytes for integer types), so an element the kernel skips shows."""
    t = torch.empty(*shape, dtype=dtype, device=device)
    t.fill_(float('nan') if dtype.is_floating_point else 0xA5)
    return t


# ---------------------------------------------------------------------------------------------- comparison
def max_err(got, want_period, chunk=CHUNK):
    """max |got[i] - want_period[i % len]| over EVERY element of got, as a float: inf if any element is NaN or infinite.
    want_period: the CPU reference for one period (any shape, float64 or exact integers)."""
    g = got.reshape(-1)
    w = want_period.reshape(-1).to(device=g.device, dtype=torch.float64)
    q, n = w.numel(), g.numel()
    per = max(1, chunk // q) * q
    worst = torch.zeros((), dtype=torch.float64, device=g.device)
    for i0 in range(0, n, per):
        i1 = min(n, i0 + per)
        d = g[i0:i1].to(torch.float64, copy=True)
        full = (i1 - i0) // q
        if full:
            d[:full * q].view(full, q).sub_(w.unsqueeze(0))
        if full * q < i1 - i0:
            d[full * q:].sub_(w[:i1 - i0 - full * q])
        d.abs_()
        m = d.max()
        worst = torch.where(torch.isfinite(m), torch.maximum(worst, m), torch.full_like(m, float('inf')))
        del d
    return float(worst)


def check_tiled(got, want_period, tol=None, atol=None, label=''):
    """Assert got == want_period tiled, within tol x max|want| (or atol); returns (err, limit)."""
    scale = float(want_period.abs().max()) if want_period.numel() else 1.0
    lim = atol if atol is not None else tol * max(scale, 1e-6)
    err = max_err(got, want_period)
    print(f'LARGE {label}: {got.numel()} elements, max err {err:.3e} (limit {lim:.3e}, scale {scale:.3e})')
    assert err <= lim, f'{label}: max err {err:.3e} > {lim:.3e} over {got.numel()} elements (scale {scale:.3e})'
    return err, lim


def check_equal(got, want, label=''):
    """A small result (a reduction's output) must equal the int64 / float64 reference exactly."""
    g = got.detach().reshape(-1).cpu().double()
    w = want.reshape(-1).double()
    assert bool(torch.isfinite(g).all()), f'{label}: non-finite result'
    err = float((g - w).abs().max())
    print(f'LARGE {label}: {g.numel()} sums, max err {err:.3e} (exact), max |want| {float(w.abs().max()):.0f}')
    assert err == 0.0, f'{label}: max err {err} against the exact reference (first at {int((g != w).nonzero()[0])})'
    return err


# ---------------------------------------------------------------------------------------------- memory
def need(nbytes):
    """Skip unless nbytes + 4 GiB of device memory are free; no test may ask for more than 40 GiB."""
    import pytest
    assert nbytes <= MAX_NEED, f'a large-extent test may need at most 40 GiB, this one states {nbytes / GIB:.1f}'
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + 4 * GIB:
        pytest.skip(f'needs {nbytes / GIB:.1f} GiB + 4 GiB of device memory, {free / GIB:.1f} GiB free')
    return nbytes


# ---------------------------------------------------------------------------------------------- one call, described by its arguments
class Tiled:
    """An input (or in-place operand) of `count` images, image b = base[b % P]."""

    def __init__(self, base_t, count, elements=None):
        self.base, self.count, self.elements = base_t, count, elements      # elements: a flat ragged length instead of whole images


class Sparse:
    """The reduced operand of a probe case: zero except at the probe images (elements: flat ragged length, the last image cut)."""

    def __init__(self, base_t, count, probe_list, elements=None):
        self.base, self.count, self.probes, self.elements = base_t, count, probe_list, elements


class Out:
    """An output the call must write completely: NaN on entry."""

    def __init__(self, *shape, dtype=torch.float32):
        self.shape, self.dtype = shape, dtype


class Small:
    """A small tensor copied to the device as it is (filters, statistics, accumulated gradients)."""

    def __init__(self, t):
        self.t = t


class Check:
    """What argument `index` must hold after the call: `want` tiled along the leading dimension (tol relative to max|want|, or
    atol), or -- exact=True -- a small tensor equal to `want`; tol with tiled=False: a small tensor within tol."""

    def __init__(self, index, want, tol=None, atol=None, exact=False, tiled=True, label=None):
        self.index, self.want, self.tol, self.atol, self.exact, self.tiled, self.label = index, want, tol, atol, exact, tiled, label


def _materialise(a, device):
    if isinstance(a, Tiled):
        if a.elements is not None:
            return tile_flat(a.base, a.elements, device)
        return tile(a.base, a.count, device)
    if isinstance(a, Sparse):
        t = sparse(a.base, a.count, a.probes, device)
        return t.reshape(-1)[:a.elements] if a.elements is not None else t
    if isinstance(a, Out):
        return fresh(*a.shape, device=device, dtype=a.dtype)
    if isinstance(a, Small):
        return a.t.clone().to(device)
    return a


def device_bytes(args):
    """Bytes the materialised arguments of a call take on the device (the comparison adds one chunk of at most 1 GiB)."""
    total = 0
    for a in args:
        if isinstance(a, (Tiled, Sparse)):
            n = a.elements if a.elements is not None else a.count * a.base[0].numel()
            total += n * a.base.element_size()
        elif isinstance(a, Out):
            n = 1
            for s in a.shape:
                n *= s
            total += n * torch.empty((), dtype=a.dtype).element_size()
    return total + 2 * CHUNK * 8


def run(K, name, args, checks, device='cuda', label=None, inputs_intact=True, expect='ok'):
    """Materialise args on `device`, call K.<name> once, check.  -> {label: max err}.  Frees everything before returning.
    inputs_intact: every Tiled argument no Check names must still equal its base, tiled, bit for bit.
    expect='rejected': the call must raise backend.KernelError (and every Out must still be untouched)."""
    import time
    label = label or name
    cuda = str(device) != 'cpu'
    sync = torch.cuda.synchronize if cuda else (lambda: None)
    dev = [_materialise(a, device) for a in args]
    sync()
    t0 = time.perf_counter()
    if expect == 'rejected':
        from tartangan_amd import backend
        try:
            getattr(K, name)(*dev)
        except backend.KernelError:
            sync()
        else:
            raise AssertionError(f'{label}: accepted a call it documents as unsupported')
        for a, d in zip(args, dev):
            if isinstance(a, Out) and a.dtype.is_floating_point:
                assert bool(torch.isnan(d).all()), f'{label}: rejected the call but wrote an output first'
        return {}
    getattr(K, name)(*dev)
    sync()
    ms = (time.perf_counter() - t0) * 1e3
    print(f'LARGE {label}: call took {ms:.1f} ms, arguments {device_bytes(args) / GIB:.2f} GiB')
    errs = {}
    checked = set()
    for c in checks:
        lab = f'{label} {c.label or "arg%d" % c.index}'
        checked.add(c.index)
        if c.exact and not c.tiled:
            errs[lab] = check_equal(dev[c.index], c.want, lab)
        elif not c.tiled:
            g, w = dev[c.index].detach().reshape(-1).cpu().double(), c.want.reshape(-1).double()
            scale = float(w.abs().max())
            lim = c.atol if c.atol is not None else c.tol * max(scale, 1e-6)
            err = float((g - w).abs().max()) if bool(torch.isfinite(g).all()) else float('inf')
            print(f'LARGE {lab}: {g.numel()} values, max err {err:.3e} (limit {lim:.3e}, scale {scale:.3e})')
            assert err <= lim, f'{lab}: max err {err:.3e} > {lim:.3e}'
            errs[lab] = err
        else:
            errs[lab] = check_tiled(dev[c.index], c.want, tol=c.tol, atol=0.0 if c.exact else c.atol, label=lab)[0]
    if inputs_intact:
        for i, a in enumerate(args):
            if isinstance(a, Tiled) and i not in checked:
                assert max_err(dev[i], a.base) == 0.0, f'{label}: modified input argument {i}'
    del dev
    if cuda:
        torch.cuda.empty_cache()
    return errs


# ---------------------------------------------------------------------------------------------- reference = the emulator on the base
class Dim:
    """A size that differs between the device call (`dev`), the reference over the P base images (`ref`) and one image (`one`)."""

    def __init__(self, dev, ref, one=None):
        self.dev, self.ref, self.one = dev, ref, one


def images(count, mult=1):
    return Dim(count * mult, P * mult, mult)


def _pick(v, which):
    return getattr(v, which) if isinstance(v, Dim) else v


def _ref_tensor(t, dtype):
    return t.to(dtype) if t.dtype.is_floating_point else t.clone()


def reference(E, name, args, dtype=torch.float64, only=None):
    """The emulator's own arguments after it ran `name` on the P base images (only=r: on base image r alone) in `dtype`."""
    which = 'ref' if only is None else 'one'
    ref = []
    for a in args:
        if isinstance(a, (Tiled, Sparse)):
            t = a.base if only is None else a.base[only:only + 1]
            ref.append(_ref_tensor(t.reshape(-1) if a.elements is not None else t, dtype))
        elif isinstance(a, Out):
            ref.append(torch.zeros([_pick(s, which) for s in a.shape], dtype=dtype if a.dtype.is_floating_point else a.dtype))
        elif isinstance(a, Small):
            ref.append(_ref_tensor(a.t, dtype))
        else:
            ref.append(_pick(a, which))
    getattr(E, name)(*ref)
    return ref


def _device_args(args):
    out = []
    for a in args:
        if isinstance(a, Out):
            a = Out(*[_pick(s, 'dev') for s in a.shape], dtype=a.dtype)
        out.append(_pick(a, 'dev'))
    return out


def run_against(K, E, name, args, outs, dtype=torch.float64, **kw):
    """One per-image call: the reference is emulator E in `dtype` on the P base images, the expected output that, tiled.
    outs: {argument index: dict(tol=) | dict(atol=) | dict(tol=, tiled=False)}."""
    ref = reference(E, name, args, dtype)
    checks = [Check(i, ref[i], label=f'arg{i}', **o) for i, o in outs.items()]
    return run(K, name, _device_args(args), checks, **kw)


def probe_want(E, name, args, outs, probe_list):
    """The exact result of a reduction over the batch whose sparse operand is nonzero at the probe images only:
    sum_r (probes on residue r) x (the emulator's float64 result on base image r alone), on top of an accumulated start."""
    counts = probe_counts(probe_list)
    want = {}
    for i in outs:
        want[i] = args[i].t.double().clone() if isinstance(args[i], Small) else None
    for r in range(P):
        if not counts[r]:
            continue
        zeroed = [Small(torch.zeros_like(a.t)) if (i in outs and isinstance(a, Small)) else a for i, a in enumerate(args)]
        ref = reference(E, name, zeroed, torch.float64, only=r)
        for i in outs:
            want[i] = counts[r] * ref[i] if want[i] is None else want[i] + counts[r] * ref[i]
    return want


def run_probe(K, E, name, args, outs, probe_list, **kw):
    """One reduction over the batch on probe data: every output in `outs` must EQUAL the reference."""
    want = probe_want(E, name, args, outs, probe_list)
    checks = [Check(i, want[i], exact=True, tiled=False, label=f'arg{i}') for i in outs]
    return run(K, name, _device_args(args), checks, **kw)


# ---------------------------------------------------------------------------------------------- the case table
class Case:
    """count: images (planes, rows, blocks) along the leading dimension; sizes: elements per image of every large operand;
    terms: for a probe reduction, (terms per probe image and output element, largest magnitude of a term)."""

    def __init__(self, count, sizes, terms=None):
        self.count, self.sizes, self.terms = count, tuple(sizes), terms

    def probes(self, offsets=OFFSETS):
        return probes(self.count, self.sizes, offsets)

    def check(self, shifts=SHIFTS, offsets=OFFSETS, bound=EXACT):
        """The period assertion for every operand and, for a reduction, the 2^24 assertion.  Arithmetic only."""
        for per in self.sizes:
            check_period(per, shifts)
        if self.terms is not None:
            check_exact(len(self.probes(offsets)) * self.terms[0], self.terms[1], bound)


IMG8 = 8 * 64 * 64                         # 8 channels at 64 x 64: 128 KiB
B_MINUS, B_PLUS, B_32, B_31E = 16383, 16385, 32768, 65540       # of 128 KiB images: 2^31 -/+ one image bytes, 2^32 bytes, 2^31 elements
assert B_MINUS * IMG8 * 4 == (1 << 31) - IMG8 * 4 and B_PLUS * IMG8 * 4 == (1 << 31) + IMG8 * 4
assert B_32 * IMG8 * 4 == 1 << 32 and B_31E * IMG8 >= 1 << 31 and B_31E > 65535
N_EW = (1 << 31) + 5                       # elementwise: ragged, so the vector body and the scalar tail both run
EW_BLOCK = 4096                            # ... seen as blocks of 4096 elements, the last one 5 long
ROWS_SM, ROWS_ATTN, COLS = (1 << 21) + 3, (1 << 20) + 3, 1024
BC_RS = 131080                             # resampling: planes of 64 x 64 on the small side, 128 x 128 on the big one
BN_B, BN_B_DBWD, BN_C, BN_HW = 8200, 4100, 16, 128 * 128

CASES = {
    # 3x3 convolutions, 8 channels at 64 x 64 unless named otherwise
    'conv3x3 B-': Case(B_MINUS, [IMG8]), 'conv3x3 B+': Case(B_PLUS, [IMG8]), 'conv3x3 B31e': Case(B_31E, [IMG8]),
    'conv3x3 8->24 B-': Case(B_MINUS, [IMG8, 3 * IMG8]), 'conv3x3 up2res B+': Case(B_PLUS, [IMG8, IMG8 // 4]),
    'conv3x3 wgrad B+': Case(B_PLUS, [IMG8, IMG8], terms=(64 * 64, 4)), 'conv3x3 wgrad B31e': Case(B_31E, [IMG8, IMG8], terms=(64 * 64, 4)),
    # 1x1 convolutions
    'conv1x1 direct 8->4': Case(65535, [IMG8, IMG8 // 2]), 'conv1x1 streaming 8->8': Case(B_31E, [IMG8]),
    'conv1x1 tiled 63x63': Case(16913, [8 * 63 * 63, 16 * 63 * 63]), 'conv1x1 wgrad B+': Case(B_PLUS, [IMG8, IMG8], terms=(64 * 64, 4)),
    'conv1x1 multi B+': Case(B_PLUS, [IMG8]), 'conv1x1 multi wgrad B+': Case(B_PLUS, [IMG8, IMG8], terms=(64 * 64, 4)),
    # stride-2 forms: low plane 32 x 32, high plane 64 x 64
    'upconv B-': Case(B_MINUS, [IMG8 // 4, IMG8]), 'upconv B+': Case(B_PLUS, [IMG8 // 4, IMG8]), 'upconv B32': Case(B_32, [IMG8 // 4, IMG8]),
    'poolconv B-': Case(B_MINUS, [IMG8, IMG8 // 2]), 'poolconv B+': Case(B_PLUS, [IMG8, IMG8 // 2]), 'poolconv B32': Case(B_32, [IMG8, IMG8 // 2]),
    'upconv wgrad B+': Case(B_PLUS, [IMG8 // 4, IMG8], terms=(64 * 64, 4)), 'poolconv wgrad B+': Case(B_PLUS, [IMG8, IMG8 // 2], terms=(64 * 64, 4)),
    # BatchNorm: 16 channels at 128 x 128
    'bn 2^31': Case(BN_B, [BN_C * BN_HW]), 'bn dbwd 2^30': Case(BN_B_DBWD, [BN_C * BN_HW]),
    # resampling and channel copies
    'resample': Case(BC_RS, [64 * 64, 128 * 128]), 'copy_channels': Case(B_31E, [7 * 4096, 8 * 4096]),
    # elementwise and scalar reductions (blocks of 4096 elements)
    'elementwise': Case((N_EW + EW_BLOCK - 1) // EW_BLOCK, [EW_BLOCK]),
    'dot sumsq': Case((N_EW + EW_BLOCK - 1) // EW_BLOCK, [EW_BLOCK], terms=(EW_BLOCK, 4)),
    # row operations
    'rows 2^21+3 x 1024': Case(ROWS_SM, [COLS]), 'rows 2^20+3 x 1024': Case(ROWS_ATTN, [COLS]),
    'channel_sum': Case(B_31E, [IMG8], terms=(64 * 64, 2)), 'channel_bcast': Case(B_31E, [IMG8]),
    'repeat sum_reps': Case(8200, [1 << 18], terms=None),
    'gemm batched': Case(2052, [1024 * 1024, 4 * 1024]),
    # image count
    'attention B=65540': Case(B_31E, [64, 16, 4 * 16, 4 * 64]),
}
