"""The dispatch ledger of csrc/conv.hip (CPU: tg_conv_dispatch launches nothing and calls no HIP function).

conv.hip compiles to some 250 kernels and ~300 lines of host code choose among them.  tests/conv_dispatch_cases.py is the
generated table of the smallest call that reaches each distinct answer of that code (tools/conv_dispatch_search.py); here the
table is held against the library: every row still gets its record, the kernels it names plus UNREACHABLE are exactly the
kernels in the library's symbol table, every value of every path flag occurs, and what the comments of the older tests say
about their shapes is asserted.  tests/test_conv_dispatch_gpu.py runs every row against the emulator.

The sweep's bounds (tools/conv_dispatch_search.py, SWEEP section): channel counts CH / S2_CH, planes PLANES / S2_PLANES, batches
BATCHES as far as MAX_BYTES = 128 MiB of tensors per call (160 MiB for the four PHASE_FORMS cases, whose arm needs 151 MiB), both placements everywhere, every single-pointer shift and every
bias / residual form on a narrow grid, the five knob sets of tests/test_knobs_gpu.py."""
import collections
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import conv_dispatch_search as S  # noqa: E402
from conv_dispatch_cases import CASES  # noqa: E402
from tartangan_amd import backend  # noqa: E402

CSRC = os.path.join(REPO, 'tartangan_amd', 'csrc')
GEO = {'Geo<4, 4, 16>': 'G4', 'Geo<8, 8, 4>': 'G8', 'Geo<16, 16, 1>': 'G16', 'Geo<8, 32, 1>': 'GX', 'Geo<4, 4, 4>': 'G4k', 'Geo<8, 8, 1>': 'G8k',
       'Geo<4, 16, 1>': 'G16k'}

# Kernels the library holds that no call can launch, each with the host condition that excludes it (checked below against the
# whole sweep).  Taking such instantiations out of the build is a change of its own.
_MTW = ('wgrad_plan: 32-channel tiles (mtw == 2) only where H * W == 64, and a plane of 64 pixels is 8 x 8 (G8) or takes the 8 x 32 '
        'geometry (GX); %s needs H * W == %d')
UNREACHABLE = {
    'conv_wgrad_kernel<G4, 1, 2>': _MTW % ('G4', 16), 'conv_wgrad_kernel<G4, 3, 2>': _MTW % ('G4', 16),
    'conv_wgrad_kernel<G16, 1, 2>': _MTW % ('G16', 256), 'conv_wgrad_kernel<G16, 3, 2>': _MTW % ('G16', 256),
    'conv_wgrad_dma_kernel<G4, 2, 16>': _MTW % ('G4', 16), 'conv_wgrad_dma_kernel<G16, 2, 16>': _MTW % ('G16', 256),
}

# Values of the recorded path flags; every family must show each value of each flag it records in some row ...
FLAG_VALUES = collections.defaultdict(lambda: ('0', '1'), xsegs=('1', '3'), ysegs=('1', '3'), gysegs=('1', '3'), items=('1',))


@pytest.fixture(scope='module')
def swept():
    """{record: (bytes, case)} of the whole sweep, once."""
    return S.search()


def library_kernels():
    """Kernel instantiations of conv.hip (and wino.h, which it includes) in the built library's symbol table, spelled as the records
    spell them."""
    src = open(os.path.join(CSRC, 'conv.hip')).read() + open(os.path.join(CSRC, 'wino.h')).read()
    defined = set(re.findall(r'__global__[^{;]*?\b(\w+_kernel)\s*\(', src))
    assert len(defined) >= 25
    out = subprocess.run(['nm', '-C', backend.LIBRARY], check=True, stdout=subprocess.PIPE, text=True).stdout
    found = set()
    for line in out.splitlines():
        if '__device_stub__' not in line:
            continue
        name = line.split('__device_stub__', 1)[1].replace('(anonymous namespace)::', '')
        name = name[:name.index('(')]
        for long, short in GEO.items():
            name = name.replace(long, short)
        name = name.replace(' >', '>')
        if name.split('<')[0] in defined:
            found.add(name)
    return found


@pytest.mark.parametrize('chunk', range(8))
def test_rows_match(chunk):
    assert len(CASES) >= 1000
    for case, record, nbytes in CASES[chunk::8]:
        assert S.query(case) == record, f'row {case}: the dispatch changed'
        assert S.tensor_bytes(case) == nbytes <= (S.MAX_BYTES_PHASES if case[1][:5] in S.PHASE_FORMS else S.MAX_BYTES), case


def test_every_kernel_is_covered():
    table = {k for _, record, _ in CASES for k in S.kernels_of(record)}
    library = library_kernels()
    print(f'ledger: {len(library)} conv kernels in the library, {len(table)} reached by {len(CASES)} rows, {len(UNREACHABLE)} unreachable; '
          f'largest row {max(n for _, _, n in CASES) / S.MiB:.1f} MiB')
    assert not (table & set(UNREACHABLE)), sorted(table & set(UNREACHABLE))
    missing, unknown = library - table - set(UNREACHABLE), (table | set(UNREACHABLE)) - library
    assert not missing, f'in the library, in no row and not in UNREACHABLE: {sorted(missing)}'
    assert not unknown, f'named by the ledger but not in the library: {sorted(unknown)}'


def test_the_table_is_what_the_search_gives(swept):
    """The committed table against a fresh search: same records, same smallest cases (regenerate it if the grid or the dispatch moved)."""
    fresh = {rec: (case, nbytes) for rec, (nbytes, case) in swept.items() if S.kernels_of(rec)}
    table = {rec: (case, nbytes) for case, rec, nbytes in CASES}
    assert len(table) == len(CASES)
    assert set(fresh) == set(table), sorted(set(fresh) ^ set(table))[:5]
    assert fresh == table


def test_unreachable_kernels_are_reached_by_nothing_in_the_sweep(swept):
    reached = {k for rec in swept for k in S.kernels_of(rec)}
    assert not (reached & set(UNREACHABLE)), sorted(reached & set(UNREACHABLE))
    assert all(len(why) > 40 for why in UNREACHABLE.values())


def test_every_flag_value_of_every_family_is_covered():
    seen = collections.defaultdict(set)
    for _, record, _ in CASES:
        for line in record.split('\n'):
            assert ';' in line, record
            for k, v in S.flags_of(line).items():
                seen[(line.split(';')[0].split('<')[0], k)].add(v)
    assert len({fam for fam, _ in seen}) >= 20
    for (fam, flag), values in sorted(seen.items()):
        assert values == set(FLAG_VALUES[flag]), f'{fam}: rows show {flag} in {sorted(values)} only'
    # residual forms of the three families tg_conv2d_fwd_up2res reaches: absent, plain, half resolution
    for fam in ('conv_fwd_kernel', 'conv_dma_kernel', 'conv_wino_dma_kernel'):
        forms = {(f['res'], f['res_up']) for _, record, _ in CASES for line in record.split('\n') if line.startswith(fam)
                 for f in [S.flags_of(line)]}
        assert forms == {('0', '0'), ('1', '0'), ('1', '1')}, (fam, forms)


def q(op, dims, knob='default', placement='aligned', bias=1, res=0):
    return S.query((op, tuple(dims) + (0,) * (8 - len(dims)), placement, bias, res, knob))


def test_what_the_older_tests_say_about_their_shapes():
    """The remarks in tests/test_guard_bands_gpu.py (FAMILIES) and tests/test_kernels_gpu.py (STEP_CONV_SHAPES), through the query.
    Two of them do not hold under the default switches; what does hold is asserted, and the child runs under TG_CONV_WINO=0 of those
    files reach what the remark names."""
    # "64 planes of 16 x 16, Cin > 16, 64 * ceil(Cout / 32) = 256 workgroups: conv_dma_kernel<G16, 32, 1, 8>" -- with Winograd off.
    # "(below the 512 the Winograd form asks for at 16 x 16, so ... the default [takes it])" does not hold: the 16-channel Winograd
    # form counts 64 * ceil(128 / 16) = 512 workgroups and takes the launch.
    shape = (64, 32, 128, 16, 16, 3)
    assert S.kernels_of(q('conv2d_fwd', shape, 'wino0')) == ['conv_dma_kernel<G16, 32, 1, 8, false>']
    assert S.kernels_of(q('conv2d_fwd', shape)) == ['conv_wino_dma_kernel<G16, 1, false, 8, false>']
    # "conv_dma_kernel<G16, 32, 1, 8> needs >= 64 images of 16x16" (the step's 128 -> 128 layer): 64 yes, 63 no
    assert S.kernels_of(q('conv2d_fwd', (64, 128, 128, 16, 16, 3), 'wino0')) == ['conv_dma_kernel<G16, 32, 1, 8, false>']
    assert S.kernels_of(q('conv2d_fwd', (63, 128, 128, 16, 16, 3), 'wino0')) == ['conv_dma_kernel<G16, 16, 1, 8, false>']
    # "8 x 8 planes, 4 images per tile, all phases in one kernel: ... 260 either way (G8)"
    assert S.kernels_of(q('upconv3x3_fwd', (520, 24, 20, 8, 8, 3))) == ['conv_upfwd_dma_kernel<G8, false>']
    assert S.kernels_of(q('upconv3x3_dgrad', (520, 24, 20, 8, 8, 3), bias=0)) == ['conv_upT_dma_kernel<G8, false>']
    assert S.kernels_of(q('upconv3x3_fwd', (520, 24, 20, 8, 8, 3), placement='shifted')) == ['conv_fwd_kernel<G8, 2, 16, 2, false>'] * 4
    # "65 * 3 = 195 forward / 65 * 2 = 130 backward, in [128, 256): the K-split form (G8k)": the forward, yes; the backward only with
    # Winograd off -- by default its 40 input channels and 258 tiles of 16 x 16 go to the pooled Winograd form
    assert S.kernels_of(q('upconv3x3_fwd', (258, 24, 40, 8, 8, 3))) == ['conv_upfwd_dma_kernel<G8k, true>']
    assert S.kernels_of(q('upconv3x3_dgrad', (258, 24, 40, 8, 8, 3), 'wino0', bias=0)) == ['conv_upT_dma_kernel<G8k, true>']
    assert S.kernels_of(q('upconv3x3_dgrad', (258, 24, 40, 8, 8, 3), bias=0)) == ['conv_poolwino_dma_kernel<G16, 2>']


def test_query_reports_every_launch_in_order_and_return_codes():
    assert q('conv2d_wgrad', (64, 128, 128, 8, 8, 3)).split('\n') == ['conv_wgrad_dma_kernel<G8, 2, 16>; prio=0 bias=1', 'wgrad_reduce_kernel; bias=1']
    assert len(S.kernels_of(q('upconv3x3_fwd', (2, 5, 7, 6, 10, 3)))) == 4
    assert q('poolconv3x3_fwd', (2, 8, 8, 8, 8, 3)) == 'rc=-2' and q('conv2d_fwd', (2, 8, 8, 8, 8, 5)) == 'rc=-2'
    assert q('conv2d_fwd', (0, 8, 8, 8, 8, 3)) == 'rc=-1'
    # the switches: explicit arguments override the environment for that call only; < 0 is what the process read (the defaults here)
    case = ('conv2d_fwd', (64, 32, 128, 16, 16, 3, 0, 0), 'aligned', 1, 0, 'default')
    if not any(k in os.environ for k in ('TG_CONV_WINO', 'TG_CONV_DMA', 'TG_DMA_PRIO')):
        assert S.query(case, (-1, -1, -1)) == S.query(case)
    assert S.query(case, (0, 0, 0)) != S.query(case, (0, 1, 0)) != S.query(case, (0, 1, 1)) != S.query(case)


def test_version_and_header():
    assert 'tg_conv_dispatch' in backend.parse_header() and len(S.OPS) == 26
    lib = S.lib()
    assert lib.tg_version() >= 109
