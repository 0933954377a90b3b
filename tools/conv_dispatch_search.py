"""The dispatch ledger's search: which kernels does csrc/conv.hip launch, and what is the smallest call that reaches each?

tg_conv_dispatch (include/tartangan_amd.h) answers for one call, from the dispatch code itself and without a GPU.  This tool
drives it over the bounded grid below (SWEEP: operations x dims x pointer placements x epilogue forms x knob sets), keeps for
every distinct answer ("record") the case with the fewest tensor bytes, and writes the table the tests share:

    python tools/conv_dispatch_search.py > tests/conv_dispatch_cases.py

tests/test_conv_dispatch.py imports sweep() and query() from here, so the ledger and the search cannot drift apart.
"""
import ctypes
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from tartangan_amd import backend  # noqa: E402

MiB = 1 << 20
MAX_BYTES = 128 * MiB             # no case of the sweep holds more tensor bytes than this (inputs + outputs + workspace) ...
MAX_BYTES_PHASES = 160 * MiB      # ... but the few cases of PHASE_FORMS below: their arm needs about 151 MiB at the least

# knob sets: (TG_CONV_WINO, TG_CONV_DMA, TG_DMA_PRIO) -- the defaults and the four sets of tests/test_knobs_gpu.py
KNOBS = {'default': (1, 1, 0), 'wino0': (0, 1, 0), 'wino2': (2, 1, 0), 'wino0_prio': (0, 1, 1), 'wino0_nodma': (0, 0, 0)}
KNOB_ENV = {k: dict(TG_CONV_WINO=str(w), TG_CONV_DMA=str(d), TG_DMA_PRIO=str(p)) for k, (w, d, p) in KNOBS.items()}


def _ops():
    src = open(backend.HEADER).read()
    return {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'#define TG_OP_(\w+) (\d+)', src)}


OPS = _ops()
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(backend.LIBRARY):
            raise RuntimeError(f'{backend.LIBRARY} is missing: build it first (python __graft_entry__.py build)')
        _LIB = ctypes.CDLL(backend.LIBRARY)
        protos = backend.parse_header()
        for name, (ret, params) in protos.items():
            if name == 'tg_conv_dispatch' or name.endswith('_workspace') and not name.startswith('tg_sn'):
                fn = getattr(_LIB, name)
                fn.restype, fn.argtypes = backend._CTYPES[ret], [backend._CTYPES[t] for t, _ in params]
    return _LIB


_PTRS = {}


def pointer_args(op):
    """Argument indices of tg_<op>'s pointer parameters, in order (bit k of tg_conv_dispatch's `unaligned` is the k-th of them)."""
    if op not in _PTRS:
        params = backend.parse_header()['tg_' + op][1]
        _PTRS[op] = [i for i, (t, a) in enumerate(params) if t.endswith('*') and a != 'stream' and 'tg_host' not in t]
    return _PTRS[op]


N_TABLE_ADDRESSES = {'conv2d_wgrad_reduce_batch': 3, 's2_wgrad_reduce_batch': 3, 'poolconv3x3_weights_batch': 3,
                     'conv1x1_wgrad_partials_batch': 5}


def mask_of(op, placement):
    """'aligned' | 'shifted' | argument index of the one shifted pointer (guarded.run_both's placements) -> `unaligned`."""
    n = N_TABLE_ADDRESSES.get(op) or len(pointer_args(op))
    if placement == 'aligned':
        return 0
    if placement == 'shifted':
        return (1 << n) - 1
    return 1 << pointer_args(op).index(placement)


def query(case, knobs=None):
    """case: (op, dims, placement, bias, res, knob set) -> the record.  knobs: explicit (wino, dma, prio), default: the set's;
    (-1, -1, -1) asks for what the process read from its environment."""
    op, (B, Cin, Cout, H, W, ks, c1, c2), placement, bias, res, knob = case
    w, d, p = KNOBS[knob] if knobs is None else knobs
    r = lib().tg_conv_dispatch(OPS[op], B, Cin, Cout, H, W, ks, c1, c2, mask_of(op, placement), bias, res, w, d, p)
    return r.decode().rstrip('\n')


def kernels_of(record):
    return [line.split(';')[0] for line in record.split('\n') if ';' in line]


def flags_of(line):
    return dict(kv.split('=') for kv in line.split(';')[1].split())


def tensor_bytes(case):
    """Bytes of every tensor argument of the call (the number the search minimises)."""
    op, (B, Cin, Cout, H, W, ks, c1, c2), _, bias, res, _ = case
    L = lib()
    lo, hi = H * W, 4 * H * W
    if op in ('conv2d_fwd', 'conv2d_fwd_up2res', 'conv2d_dgrad'):
        n = B * (Cin + Cout) * lo + Cout * Cin * ks * ks + (B * Cout * (lo // 4 if op.endswith('up2res') else lo) if res else 0)
    elif op in ('conv2d_wgrad', 'conv2d_wgrad_partials', 'conv2d_wgrad_reduce_batch'):
        n = B * (Cin + Cout) * lo + Cout * Cin * ks * ks + L.tg_conv2d_wgrad_workspace(B, Cin, Cout, H, W, ks) // 4
    elif op in ('upconv3x3_fwd', 'upconv3x3_dgrad'):
        n = B * Cin * lo + B * Cout * hi * (2 if res else 1) + 16 * Cout * Cin
    elif op in ('poolconv3x3_fwd', 'poolconv3x3_dgrad'):
        n = B * Cin * hi + B * Cout * lo * (2 if res else 1) + 16 * Cout * Cin
    elif op in ('upconv3x3_wgrad', 'upconv3x3_wgrad_partials'):
        n = B * Cin * lo + B * Cout * hi + L.tg_upconv3x3_wgrad_workspace(B, Cin, Cout, H, W) // 4
    elif op in ('poolconv3x3_wgrad', 'poolconv3x3_wgrad_partials'):
        n = B * Cin * hi + B * Cout * lo + L.tg_poolconv3x3_wgrad_workspace(B, Cin, Cout, H, W) // 4
    elif op == 's2_wgrad_reduce_batch':
        n = B * (Cin * (lo if ks else hi) + Cout * (hi if ks else lo)) + (L.tg_upconv3x3_wgrad_workspace if ks else L.tg_poolconv3x3_wgrad_workspace)(B, Cin, Cout, H, W) // 4
    elif op.startswith('conv1x1_multi') or op == 'conv1x1_wgrad_partials_batch':
        C = Cout + c1 + c2
        n = B * (Cin + C) * lo + C * Cin + L.tg_conv2d_wgrad_workspace(B, Cin, C, H, W, 1) // 4
    else:                                                  # filter transforms: a few filters
        n = 64 * Cout * max(Cin, 4)
    return 4 * n


# ------------------------------------------------------------------------------------------------------------- the sweep
# Channel counts: below / at / between the 4-, 8-, 16- and 32-multiples the conditions test, the 48 / 64 tile switches.
CH = (3, 4, 8, 12, 16, 20, 32, 40, 48, 64, 128)
# Planes: the four tile geometries (4x4, 8x8, 16x16, 8 rows x 32), whole and ragged tiles, W % 4 != 0, odd; 4 x 16: 64 pixels that
# are no 8 x 8 plane (the weight gradient's 32-channel tiles on the 8 x 32 geometry).
PLANES = ((4, 4), (8, 8), (16, 16), (8, 32), (32, 32), (64, 64), (12, 20), (9, 11), (16, 64), (4, 16))
# Batches: small, odd (B % 2, ragged image groups), and the neighbours of the workgroup thresholds (128 / 192 / 256 / 512 / 768
# workgroups over 1, 4 or 16 images per tile and 1 .. 8 channel tiles), as far as MAX_BYTES allows.
BATCHES = (1, 2, 3, 5, 8, 16, 17, 24, 32, 33, 48, 63, 64, 65, 96, 128, 129, 192, 256, 257, 384, 512, 513, 768, 1024, 1536, 2048,
           3072, 4096, 6144, 8192, 12288)
S2_PLANES = ((4, 4), (8, 8), (16, 16), (8, 32), (32, 32), (6, 10), (16, 64))          # the LOW-resolution plane
S2_CH = (5, 8, 16, 20, 24, 32, 40, 64, 128)
FWD_FORMS = ((1, 0), (0, 0), (0, 1), (1, 1))               # (bias, residual)
# The 64-channel tiles of the per-phase form of tg_upconv3x3_fwd (launch_fwd_geo: from 768 workgroups of 64 channels x 256 low-resolution
# pixels, i.e. 768 x 256 x 4 high-resolution pixels per output channel): cheapest with the fewest channels that still take 32-row tiles
# (Cout = 49 > 48) and a thin input.  4 x 4 planes always run per phase; 8 x 8 and 16 x 16 ones when y sits off an 8-byte boundary.
PHASE_FORMS = ((12288, 5, 49, 4, 4), (12287, 5, 49, 4, 4), (3072, 5, 49, 8, 8), (768, 5, 49, 16, 16))
ALL_KNOBS = tuple(KNOBS)


def _placements(op, narrow):
    return ('aligned', 'shifted') + (tuple(pointer_args(op)) if narrow and op not in N_TABLE_ADDRESSES else ())


def sweep():
    """Every case of the search.  The wide grid runs each operation with both placements, bias and no residual (fwd) / bias
    (wgrad); the narrow grid (the first batches, a few channel counts) adds every single-pointer shift and every epilogue form."""
    def dims_grid(batches, chans_in, chans_out, planes):
        for H, W in planes:
            for B in batches:
                for Cin in chans_in:
                    for Cout in chans_out:
                        yield B, Cin, Cout, H, W

    def emit(op, d, ks, narrow, knobs):
        fwd = op in ('conv2d_fwd', 'upconv3x3_fwd', 'poolconv3x3_fwd')
        forms = (FWD_FORMS if fwd else ((1, 1), (0, 1)) if op == 'conv2d_fwd_up2res' else ((1, 0), (0, 0)) if 'wgrad' in op else ((0, 0),))
        for pl in _placements(op, narrow):
            for bias, res in (forms if narrow else forms[:1]):
                for knob in knobs:
                    case = (op, d + (ks, 0, 0), pl, bias, res, knob)
                    if tensor_bytes(case) <= MAX_BYTES:
                        yield case

    narrow_b, narrow_c, narrow_p = (2, 64), (5, 32), ((8, 8), (16, 16), (12, 20))
    for ks in (3, 1):
        knobs = ALL_KNOBS if ks == 3 else ('default',)
        for op in ('conv2d_fwd', 'conv2d_dgrad', 'conv2d_wgrad'):
            for d in dims_grid(BATCHES, CH, CH, PLANES):
                yield from emit(op, d, ks, False, knobs)
            for d in dims_grid(narrow_b, narrow_c, narrow_c, narrow_p):
                yield from emit(op, d, ks, True, knobs)
    for d in dims_grid(narrow_b, narrow_c, narrow_c, narrow_p):            # (the kernels of conv2d_fwd with res_up = 1)
        yield from emit('conv2d_fwd_up2res', d, 3, True, ALL_KNOBS)
    for op in ('upconv3x3_fwd', 'upconv3x3_dgrad', 'poolconv3x3_fwd', 'poolconv3x3_dgrad', 'upconv3x3_wgrad', 'poolconv3x3_wgrad'):
        for d in dims_grid(BATCHES, S2_CH, S2_CH, S2_PLANES):
            yield from emit(op, d, 3, False, ALL_KNOBS)
        for d in dims_grid((2, 128, 258, 520), narrow_c, narrow_c, ((8, 8), (16, 16), (6, 10))):     # (the one-kernel forms need >= 128 / 256 workgroups)
            yield from emit(op, d, 3, True, ALL_KNOBS)
    for d in PHASE_FORMS:
        for pl in ('aligned', 'shifted'):
            case = ('upconv3x3_fwd', d + (3, 0, 0), pl, 1, 0, 'default')
            assert tensor_bytes(case) <= MAX_BYTES_PHASES
            yield case
    # the two-step forms and the filter transforms: one kernel each besides the stage-1 kernels the one-call forms reach
    small = [(2, 5, 7, 12, 20), (3, 16, 16, 16, 16), (2, 32, 40, 8, 8)]
    for d in small:
        for ks in (1, 3):
            for op in ('conv2d_wgrad_partials', 'conv2d_wgrad_reduce_batch'):
                yield from emit(op, d, ks, False, ('default',))
        for op in ('upconv3x3_wgrad_partials', 'poolconv3x3_wgrad_partials'):
            yield from emit(op, d, 3, False, ('default',))
        for mode in (0, 1):
            yield from emit('s2_wgrad_reduce_batch', d, mode, False, ('default',))
    for Cout, Cin in ((5, 7), (16, 16), (33, 40)):
        for op in ('upconv3x3_weights', 'upconv3x3_weights_t', 'upconv3x3_weights_pair', 'poolconv3x3_weights', 'poolconv3x3_weights_batch'):
            for pl in ('aligned', 'shifted'):
                yield (op, (0, Cin, Cout, 0, 0, 0, 0, 0), pl, 0, 0, 'default')
        for op in ('rgb_compose_fwd', 'rgb_compose_bwd'):
            for pl in ('aligned', 'shifted'):
                yield (op, (0, Cin, Cout, 0, 0, 3, 0, 0), pl, 0, 0, 'default')        # (Cout, C = Cin, Cimg = ks)
    # the three-segment 1x1 forms and the grouped stage 1: (B, Cin, c0, H, W, c1, c2)
    for B, Cin, c0, H, W, c1, c2 in ((2, 16, 2, 4, 4, 2, 8), (2, 20, 2, 12, 12, 2, 10), (3, 40, 8, 8, 8, 8, 16), (2, 8, 16, 16, 16, 24, 24),
                                     (2, 64, 4, 8, 8, 4, 4), (2, 8, 8, 6, 6, 8, 8)):
        for op in ('conv1x1_multi_fwd', 'conv1x1_multi_dgrad', 'conv1x1_multi_wgrad', 'conv1x1_wgrad_partials_batch'):
            for pl in ('aligned', 'shifted'):
                for bias in ((0, 1) if op.endswith('batch') else (0,)):
                    yield (op, (B, Cin, c0, H, W, 1, c1, c2), pl, bias, 0, 'default')
    for B, Cin, Cout, H, W in ((2, 8, 8, 8, 8), (3, 40, 33, 4, 4), (2, 16, 40, 12, 12)):      # ... and its one-tensor rows
        for bias in (0, 1):
            yield ('conv1x1_wgrad_partials_batch', (B, Cin, Cout, H, W, 1, 0, 0), 'aligned', bias, 0, 'default')


def search():
    """-> {record: (bytes, case)}: the smallest case of the sweep for every distinct record."""
    best = {}
    for case in sweep():
        rec = query(case)
        key = (tensor_bytes(case), repr(case))
        if rec not in best or key < best[rec][0]:
            best[rec] = (key, case)
    return {rec: (key[0], case) for rec, (key, case) in best.items()}


def main():
    best = search()
    rows = sorted(((case, rec, nbytes) for rec, (nbytes, case) in best.items() if kernels_of(rec)), key=lambda r: (r[0][0], r[2], repr(r[0])))
    out = ['"""GENERATED by tools/conv_dispatch_search.py -- do not edit; regenerate with',
           '    python tools/conv_dispatch_search.py > tests/conv_dispatch_cases.py',
           'One row per distinct answer of tg_conv_dispatch over the search\'s grid, each the case with the fewest tensor bytes:',
           '(operation, (B, Cin, Cout, H, W, ks, c1, c2), placement, bias, residual, knob set), the expected record, tensor bytes."""',
           'CASES = [']
    for case, rec, nbytes in rows:
        out.append(f'    ({case!r},\n     {rec!r}, {nbytes}),')
    out.append(']')
    print('\n'.join(out))
    print(f'{len(rows)} rows, {len({k for _, r, _ in rows for k in kernels_of(r)})} kernels, largest {max(r[2] for r in rows) / MiB:.1f} MiB',
          file=sys.stderr)


if __name__ == '__main__':
    main()
