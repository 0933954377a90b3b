"""tg_conv1x1_wgrad_partials_batch: stage 1 of many 1x1 weight gradients in one launch.  Grouped stage 1 plus one batched reduce
against the one-call forms (tg_conv2d_wgrad, tg_conv1x1_multi_wgrad), bit for bit: same body, same plan, same summation order.
The mixed table also goes through the guard-banded harness against the emulator, aligned (accepted) and shifted (rejected).

(This file sorts in front of test_guard_bands_gpu.py on purpose: that file's completeness test wants every entry point with a
pointer parameter to have gone through guarded.run_both earlier in the same process.)"""
import pytest
import torch

from grouped_wgrad_cases import CASES, FIELDS, GroupedEmulator
from guarded import HostTable, Per, rnd, run_both, workspace

pytestmark = pytest.mark.gpu
GE = GroupedEmulator()


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    backend._set_backend_for_testing(None)
    return backend.get()


class Item:
    """One layer: operands on the device, the one-call form's result (accumulated onto random gradients), and fresh copies of
    those gradients for the two-step path."""

    def __init__(self, K, seed, B, Cin, cs, H, W, bias, gw=None, gb=None):
        self.dims, self.cs, self.bias = (B, Cin, sum(cs), H, W), cs, bias
        C = sum(cs)
        self.x = rnd(B, Cin, H, W, seed=seed).cuda()
        self.gys = [rnd(B, c, H, W, seed=100 + 10 * seed + k).cuda() for k, c in enumerate(cs)]
        self.nbytes = K.conv2d_wgrad_workspace(B, Cin, C, H, W, 1)
        self.ws = workspace(self.nbytes).cuda()
        self.gw = rnd(C, Cin, seed=200 + seed).cuda() if gw is None else gw
        self.gb = rnd(C, seed=300 + seed).cuda() if gb is None else gb

    def one_call(self, K, gw, gb):
        B, Cin, C, H, W = self.dims
        ws = workspace(self.nbytes).cuda()
        if len(self.cs) == 1:
            K.conv2d_wgrad(self.x, self.gys[0], gw, gb if self.bias else None, ws, ws.numel() * 4, B, Cin, C, H, W, 1, 1)
        else:
            K.conv1x1_multi_wgrad(self.x, *self.gys, gw, ws, ws.numel() * 4, *self.cs, B, Cin, H, W, 1)

    def stage1_row(self, ws_bytes=None):
        B, Cin, C, H, W = self.dims
        ptrs = [g.data_ptr() for g in self.gys] + [0] * (3 - len(self.gys))
        widths = list(self.cs) + [0] * (3 - len(self.cs))
        return [self.x.data_ptr(), *ptrs, self.ws.data_ptr(), self.nbytes if ws_bytes is None else ws_bytes, *widths, B, Cin, H, W, 1,
                int(self.bias)]

    def reduce_row(self):
        B, Cin, C, H, W = self.dims
        return [self.ws.data_ptr(), self.gw.data_ptr(), self.gb.data_ptr() if self.bias else 0, B, Cin, C, H, W, 1, 1]


def table(rows):
    return torch.tensor(rows, dtype=torch.int64)


def check_two_steps_equal_one_call(K, items):
    want = []
    for it in items:
        a, ab = it.gw.clone(), it.gb.clone()
        it.one_call(K, a, ab)
        want.append((a, ab))
    K.conv1x1_wgrad_partials_batch(table([it.stage1_row() for it in items]), len(items))
    K.conv2d_wgrad_reduce_batch(table([it.reduce_row() for it in items]), len(items))
    torch.cuda.synchronize()
    for n, (it, (a, ab)) in enumerate(zip(items, want)):
        assert torch.equal(a, it.gw), (n, it.dims, float((a - it.gw).abs().max()))
        assert torch.equal(ab, it.gb), (n, it.dims)           # (no bias: both untouched)


@pytest.mark.parametrize('case', sorted(CASES))
def test_one_item_is_bit_identical_to_the_one_call_form(K, case):
    assert K.conv1x1_wgrad_batch_supported(*Item(K, 1, *CASES[case]).dims)
    check_two_steps_equal_one_call(K, [Item(K, 1, *CASES[case])])


def test_mixed_table_in_one_call(K):
    """g: every case in one table -- all four <MT, NT> variants, one and three gy tensors, with and without bias in ONE launch."""
    check_two_steps_equal_one_call(K, [Item(K, i, *CASES[c]) for i, c in enumerate(sorted(CASES))])


def test_mixed_table_behind_guard_bands(K):
    """g again through the guarded harness: nothing outside the operands and the exact workspaces is touched; the finished gradients
    agree with the emulator (tolerance of tg_conv2d_wgrad's own parity test); one element off, the table is rejected unwritten."""
    rows, s1_scratch = [], []
    for r, c in enumerate(sorted(CASES)):
        B, Cin, cs, H, W, bias = CASES[c]
        gys = [rnd(B, k, H, W, seed=100 + 10 * r + n) for n, k in enumerate(cs)] + [None] * (3 - len(cs))
        nbytes = K.conv2d_wgrad_workspace(B, Cin, sum(cs), H, W, 1)
        rows.append([rnd(B, Cin, H, W, seed=r), *gys, workspace(nbytes), nbytes, *(list(cs) + [0] * (3 - len(cs))), B, Cin, H, W, 1, int(bias)])
        s1_scratch.append((r, 4))
    run_both(K, 'conv1x1_wgrad_partials_batch', [HostTable(rows, scratch=s1_scratch), len(rows)], [], placement='shifted', expect='rejected',
             emulator=GE)
    # the emulator's workspaces hold ONE partial each, the device's S of them: each side reduces its own
    emu = [[t.clone() if torch.is_tensor(t) else t for t in row] for row in rows]
    for row in emu:
        nb = GE.conv2d_wgrad_workspace(row[9], row[10], row[6] + row[7] + row[8], row[11], row[12], 1)
        row[4], row[5] = workspace(nb), nb
    GE.conv1x1_wgrad_partials_batch(table([[t.data_ptr() if torch.is_tensor(t) else int(t or 0) for t in row] for row in emu]), len(emu))
    dev = run_both(K, 'conv1x1_wgrad_partials_batch', [HostTable(rows, scratch=s1_scratch), len(rows)], [], emulator=GE)[0]
    red, outs = [], []
    for r, (row, erow) in enumerate(zip(rows, emu)):
        B, Cin, H, W, bias = row[9], row[10], row[11], row[12], row[14]
        C = row[6] + row[7] + row[8]
        red.append([Per(erow[4], dev[(r, 4)].cpu()), rnd(C, Cin, seed=200 + r), rnd(C, seed=300 + r) if bias else None, B, Cin, C, H, W, 1, 1])
        outs += [(r, 1)] + ([(r, 2)] if bias else [])
    run_both(K, 'conv2d_wgrad_reduce_batch', [HostTable(red, outs=outs, accum=outs), len(red)], [], tol=5e-5, emulator=GE)


def test_more_items_than_one_argument_block_holds(K):
    """h: 45 small items -- more than the 40 one launch carries."""
    names = sorted(CASES)
    check_two_steps_equal_one_call(K, [Item(K, i, *CASES[names[i % len(names)]]) for i in range(45)])


def test_one_gradient_twice_in_two_reduce_rounds(K):
    """i: two contributions to ONE gradient (the discriminator's real | fake pass and its R1 term): one grouped stage 1, then
    contribution k in reduce launch k == two accumulating one-call forms in the same order."""
    first = Item(K, 1, *CASES['d'])
    second = Item(K, 2, *CASES['d'], gw=first.gw, gb=first.gb)
    a, ab = first.gw.clone(), first.gb.clone()
    first.one_call(K, a, ab)
    second.one_call(K, a, ab)
    K.conv1x1_wgrad_partials_batch(table([first.stage1_row(), second.stage1_row()]), 2)
    K.conv2d_wgrad_reduce_batch(table([first.reduce_row()]), 1)
    K.conv2d_wgrad_reduce_batch(table([second.reduce_row()]), 1)
    torch.cuda.synchronize()
    assert torch.equal(a, first.gw) and torch.equal(ab, first.gb)


def _rejected_unwritten(K, items, rows, code):
    """The call fails with ``code`` and no workspace of the table changed (they hold a sentinel)."""
    from tartangan_amd import backend
    for it in items:
        it.ws.fill_(-7.0)
    torch.cuda.synchronize()
    with pytest.raises(backend.KernelError, match=f'code {code}$'):
        K.conv1x1_wgrad_partials_batch(table(rows), len(rows))
    torch.cuda.synchronize()
    for it in items:
        assert bool((it.ws == -7.0).all())


def test_rejections_leave_nothing_written(K):
    good = [Item(K, i, *CASES[c]) for i, c in enumerate('ad')]
    ok_rows = [it.stage1_row() for it in good]
    # a 6 x 6 plane: H W % 16 != 0 (the query says so too); the good rows in front of it must not run either
    assert not K.conv1x1_wgrad_batch_supported(2, 16, 16, 6, 6)
    bad = Item(K, 5, 2, 16, (16,), 6, 6, False)
    _rejected_unwritten(K, good + [bad], ok_rows + [bad.stage1_row()], -2)
    # one operand one element off: x, then gy, then the workspace
    for field in (0, 1, 4):
        it = Item(K, 6, *CASES['d'])
        row = it.stage1_row()
        row[field] += 4
        _rejected_unwritten(K, good + [it], ok_rows + [row], -2)
    # a workspace 4 bytes short
    it = Item(K, 7, *CASES['d'])
    _rejected_unwritten(K, good + [it], ok_rows + [it.stage1_row(ws_bytes=it.nbytes - 4)], -3)
    # the same through the guarded harness: an exact workspace of nbytes - 4, its guard right behind it
    B, Cin, cs, H, W, bias = CASES['d']
    nbytes = K.conv2d_wgrad_workspace(B, Cin, cs[0], H, W, 1) - 4
    rows = [[rnd(B, Cin, H, W), rnd(B, cs[0], H, W, seed=3), None, None, workspace(nbytes), nbytes, cs[0], 0, 0, B, Cin, H, W, 1, 1]]
    run_both(K, 'conv1x1_wgrad_partials_batch', [HostTable(rows, scratch=[(0, 4)]), 1], [], expect='rejected', emulator=GE)
    # ks = 3 has no grouped form; three widths need three tensors
    it = Item(K, 8, *CASES['d'])
    row = it.stage1_row()
    row[13] = 3
    _rejected_unwritten(K, [it], [row], -2)
    row = it.stage1_row()
    row[7], row[8] = 4, 4
    _rejected_unwritten(K, [it], [row], -1)
    # the table is host memory
    with pytest.raises(RuntimeError, match='CPU int64'):
        K.conv1x1_wgrad_partials_batch(table(ok_rows).cuda(), len(ok_rows))


def test_empty_table_is_ok_and_launches_nothing(K):
    assert K.conv1x1_wgrad_partials_batch(torch.zeros(0, FIELDS, dtype=torch.int64), 0) == 0
    assert K.conv1x1_wgrad_partials_batch(None, 0) == 0
    torch.cuda.synchronize()
