"""The guard-band harness (tests/guarded.py) shown to catch what it claims, on the CPU: the emulator stands in for the
device, once unmodified (must pass at every placement kind) and once per defect (must fail, naming the argument and the
kind of violation).  The defective stand-ins are Python stubs over CPU tensors; nothing here runs a faulty kernel."""
import pytest
import torch

from emulator import Emulator
from guarded import HostTable, Per, rnd, run_both, workspace
from tartangan_amd import backend

E = Emulator()
N = 37


def _beyond(t, k):
    """The element k places past the end (k >= 1) or before the start (k <= -1) of a placed view: its guard."""
    off = t.storage_offset() + (t.numel() + k - 1 if k > 0 else k)
    return torch.as_strided(t, (1,), (1,), off)


class Defective(Emulator):
    def __init__(self, defect):
        self.defect = defect

    def add(self, a, b, out, n):
        d = self.defect
        if d == 'adds_into_fresh':
            out.add_(a + b)
            return 0
        super().add(a, b, out, n)
        if d == 'past_end':
            _beyond(out, 1).fill_(1.0)
        elif d == 'before_start':
            _beyond(out, -1).fill_(1.0)
        elif d == 'reads_past_input':
            out.view(-1)[-1] += _beyond(b, 1)[0]
        elif d == 'modifies_input':
            a.view(-1)[3] = 0.0
        elif d == 'writes_then_fails':
            raise backend.KernelError('tg_add failed with code -2')
        return 0

    def dot(self, a, b, alpha, out, ws, n, accumulate):
        super().dot(a, b, alpha, out, ws, n, accumulate)
        _beyond(ws, 1).fill_(0.0)
        return 0


def _add(K, **kw):
    return run_both(K, 'add', [rnd(N), rnd(N, seed=1), torch.zeros(N), N], [2], atol=0.0, device='cpu', **kw)


@pytest.mark.parametrize('placement', ['aligned', 'shifted', 0, 1, 2])
@pytest.mark.parametrize('defect,argument,kind', [
    ('past_end', 'out (argument 2)', 'guard past the end of'),
    ('before_start', 'out (argument 2)', 'guard before the start of'),
    ('reads_past_input', 'out (argument 2)', 'read outside an input'),
    ('adds_into_fresh', 'out (argument 2)', 'depends on its content on entry'),
    ('modifies_input', 'a (argument 0)', 'modified input'),
])
def test_each_defect_is_caught_and_named(defect, argument, kind, placement):
    with pytest.raises(AssertionError) as e:
        _add(Defective(defect), placement=placement)
    msg = str(e.value)
    assert msg.startswith('add [') and argument in msg and kind in msg, msg


def test_guard_report_gives_side_and_offsets():
    with pytest.raises(AssertionError) as e:
        _add(Defective('past_end'))
    assert 'first at offset 1, last at offset 1' in str(e.value)
    with pytest.raises(AssertionError) as e:
        _add(Defective('before_start'))
    assert 'first at offset -1, last at offset -1' in str(e.value)


@pytest.mark.parametrize('placement', ['aligned', 'shifted', 4])
def test_write_past_the_declared_workspace_bytes_is_caught(placement):
    nbytes = E.reduce_workspace(N)
    ws = workspace(nbytes)
    assert ws.numel() * 4 == nbytes                       # exact: the guard starts right behind the declared bytes
    args = [rnd(N), rnd(N, seed=1), 0.5, torch.zeros(()), ws, N, 0]
    run_both(E, 'dot', args, [3], tol=1e-5, device='cpu', placement=placement)
    with pytest.raises(AssertionError) as e:
        run_both(Defective(None), 'dot', args, [3], tol=1e-5, device='cpu', placement=placement)
    assert 'guard past the end of workspace (argument 4)' in str(e.value) and 'first at offset 1,' in str(e.value)


def test_rejected_calls_must_raise_and_leave_everything_untouched():
    class Rejects(Emulator):
        def add(self, a, b, out, n):
            raise backend.KernelError('tg_add failed with code -2')

    _add(Rejects(), expect='rejected', placement=['aligned', 'shifted', 1])
    with pytest.raises(AssertionError) as e:
        _add(Defective('writes_then_fails'), expect='rejected')
    assert 'rejected the call but wrote out (argument 2)' in str(e.value)
    with pytest.raises(AssertionError) as e:
        _add(E, expect='rejected')
    assert 'accepted a call it documents as unsupported' in str(e.value)


@pytest.mark.parametrize('placement', ['aligned', 'shifted', 'each'])
def test_clean_emulator_passes_every_placement(placement):
    def run(name, args, outs, **kw):
        ptrs = [i for i, a in enumerate(args) if torch.is_tensor(a)]
        run_both(E, name, args, outs, device='cpu', placement=ptrs if placement == 'each' else placement, **kw)

    run('add', [rnd(N), rnd(N, seed=1), torch.zeros(N), N], [2], atol=0.0)
    B, Cin, Cout, H, W = 2, 3, 5, 6, 7
    x, gy = rnd(B, Cin, H, W), rnd(B, Cout, H, W, seed=3)
    ws = workspace(E.conv2d_wgrad_workspace(B, Cin, Cout, H, W, 3))
    for acc in (0, 1):          # fresh (NaN on entry) and read-modify-write (values kept) outputs
        run('conv2d_wgrad', [x, gy, rnd(Cout, Cin, 3, 3, seed=9), rnd(Cout, seed=10), ws, ws.numel() * 4, B, Cin, Cout, H, W, 3, acc],
            [2, 3], tol=1e-5)
    nbt = torch.tensor(41, dtype=torch.int64)                # an int64 scalar that is read-modify-write
    run('bn_train_stats', [rnd(B, Cin, H * W), torch.zeros(Cin), torch.zeros(Cin), rnd(Cin), 1 + torch.rand(Cin), nbt, 0.1, 1e-5,
                           workspace(E.bn_workspace(B, Cin, H * W)), B, Cin, H * W, 1], [1, 2, 3, 4, 5], tol=1e-6)
    idx = torch.zeros(3, 3, 4, dtype=torch.uint8)            # a uint8 output
    run('maxpool2_fwd', [rnd(3, 6, 8), torch.zeros(3, 3, 4), idx, 3, 6, 8], [1, 2], atol=0.0)
    run('gemm', [rnd(1, 3, 4), rnd(1, 4, 5, seed=1), rnd(1, 3, 5, seed=2), None, 3, 5, 4, 4, 5, 5, 0, 0, 1, 12, 20, 15, 1.0], [2], tol=1e-6)


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
def test_host_table_tensors_are_placed_and_checked(placement):
    B, Cin, Cout, H, W, ks = 2, 3, 5, 6, 7, 3
    x, gy = rnd(B, Cin, H, W), rnd(B, Cout, H, W, seed=3)
    ws = workspace(E.conv2d_wgrad_workspace(B, Cin, Cout, H, W, ks))
    E.conv2d_wgrad_partials(x, gy, ws, ws.numel() * 4, B, Cin, Cout, H, W, ks, 1)
    rows = [[Per(ws, ws.clone()), rnd(Cout, Cin, ks, ks, seed=9), rnd(Cout, seed=10), B, Cin, Cout, H, W, ks, 1],
            [ws, torch.zeros(Cout, Cin, ks, ks), None, B, Cin, Cout, H, W, ks, 0]]
    table = HostTable(rows, outs=[(0, 1), (0, 2), (1, 1)], accum=[(0, 1), (0, 2)])
    got = run_both(E, 'conv2d_wgrad_reduce_batch', [table, 2], [], device='cpu', placement=placement)
    want = torch.nn.grad.conv2d_weight(x, (Cout, Cin, ks, ks), gy, padding=1)
    assert torch.allclose(got[0][(1, 1)], want, rtol=1e-5, atol=1e-5)

    class Overruns(Emulator):
        def conv2d_wgrad_reduce_batch(self, items, n_items):
            super().conv2d_wgrad_reduce_batch(items, n_items)
            import ctypes
            ctypes.c_float.from_address(int(items[1][1]) + 4 * Cout * Cin * ks * ks).value = 0.0
            return 0

    with pytest.raises(AssertionError) as e:
        run_both(Overruns(), 'conv2d_wgrad_reduce_batch', [table, 2], [], device='cpu', placement=placement)
    assert 'guard past the end of items[1][1] (host table)' in str(e.value)

