"""Guard-banded placement of kernel arguments: what a kernel touches OUTSIDE its tensors.  TEST INFRASTRUCTURE ONLY.

``run_both`` runs one entry point of include/tartangan_amd.h on the emulator (once) and on the device (once per
placement) and compares.  On the device side every tensor argument is a contiguous view into the interior of a larger
buffer of the same dtype, ``GUARD`` elements clear of either end:

  * placement 'aligned': every view starts 16-byte aligned (asserted); 'shifted': every view starts one element further
    (4 bytes off for floats), which sends the call down the unaligned dispatch paths; an integer: that pointer argument
    alone is shifted;
  * the guards of inputs hold NaN (an outside read that reaches the result shows as NaN), those of outputs and workspaces
    a fixed quiet-NaN bit pattern that arithmetic does not produce, integer tensors a fixed byte pattern; after the call
    every guard must be bit-identical (compared as integers) to what was put there;
  * an output whose previous content must not matter is handed over filled with NaN instead of the zeros the test passed;
    read-modify-write outputs (taken from the header's documentation: ``ACCUM`` below, or ``accum=``) keep their values;
  * workspaces are exactly ``ceil(nbytes / 4)`` floats, the guard right behind them, also NaN on entry;
  * tensors whose addresses travel in a host table (``HostTable``) are placed and checked like arguments;
  * expect='rejected': the call must raise ``backend.KernelError`` and leave every output, workspace and guard as it was.

What this cannot see: a stray READ whose value is discarded.  Nothing here places a tensor against unmapped memory or
otherwise tries to turn a stray access into a fault; the guards are ordinary memory that is compared afterwards.
"""

import torch

from emulator import Emulator

E = Emulator()
GUARD = 1024                      # elements each side: longer than any tile row or float4 tail a kernel here can overshoot by

_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64}
_OUT_SENTINEL = {torch.float32: 0x7FC5A5A5, torch.float64: 0x7FF85A5A5A5A5A5A}       # quiet NaNs with a payload
_FRESH_FILL = {torch.float32: 0x7FC0F111, torch.float64: 0x7FF80000F111F111}
_INT_PATTERN = {torch.uint8: 0xA5, torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5A5A5A5A5B}   # bytes 0xA5 throughout

SEEN = set()                      # entry points that went through run_both in this process (the completeness test reads it)


def workspace(nbytes):
    """Exactly ceil(nbytes / 4) floats; run_both puts the guard right behind them and fills them with NaN on the device."""
    t = torch.zeros((int(nbytes) + 3) // 4)
    t._is_ws = True
    return t


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return torch.randn(*shape, generator=g) * scale


class Per:
    """A tensor whose content differs between the two sides (a stage-1 workspace: the emulator's layout is not the device's)."""

    def __init__(self, emulator, device):
        self.emulator, self.device = emulator, device


class HostTable:
    """A host array of 64-bit words some of which are device addresses (tg_*_reduce_batch, tg_poolconv3x3_weights_batch).
    rows: lists of ints / CPU tensors / Per / None (-> 0); outs, accum, scratch: (row, column) positions of tensors with
    that role.  Every tensor in it is placed behind guards and checked like an argument."""

    def __init__(self, rows, outs=(), accum=(), scratch=(), tol=None):
        self.rows, self.outs, self.accum, self.scratch, self.tol = [list(r) for r in rows], list(outs), set(accum), set(scratch), tol

    def cells(self):
        return [((r, c), v) for r, row in enumerate(self.rows) for c, v in enumerate(row) if torch.is_tensor(v) or isinstance(v, Per)]

    def build(self, tensors):
        return torch.tensor([[tensors[(r, c)].data_ptr() if (r, c) in tensors else int(v or 0) for c, v in enumerate(row)]
                             for r, row in enumerate(self.rows)], dtype=torch.int64)


def _flag(name, *outs):
    return lambda a: outs if a[name] else ()


# Outputs that are read-modify-write BY THE HEADER'S DOCUMENTATION of the entry point: argument names, given the call's arguments.
ACCUM = {
    'conv2d_wgrad': _flag('accumulate', 'gw', 'gbias'), 'poolconv3x3_wgrad': _flag('accumulate', 'gw', 'gbias'),
    'upconv3x3_wgrad': _flag('accumulate', 'gw', 'gbias'), 'conv1x1_multi_wgrad': _flag('accumulate', 'gw'),
    'rgb_compose_bwd': _flag('accumulate', 'gw1', 'gb1', 'gw3'), 'channel_sum': _flag('accumulate', 'out'),
    'dot': _flag('accumulate', 'out'), 'gemm': _flag('beta', 'C'),
    'bn_train_stats': lambda a: ('running_mean', 'running_var', 'num_batches_tracked'),
    'bn_train_fwd': lambda a: ('running_mean', 'running_var', 'num_batches_tracked'),
    'bn_train_fwd_groups': lambda a: ('running_mean', 'running_var', 'num_batches_tracked'),
    'bn_sync_stats_finish': lambda a: ('running_mean', 'running_var', 'num_batches_tracked'),
    'bn_act_bwd': _flag('accumulate', 'ggamma', 'gbeta'), 'bn_act_bwd_groups': _flag('accumulate', 'ggamma', 'gbeta'),
    'bn_sync_bwd_finish': _flag('accumulate', 'ggamma', 'gbeta'),
    'bn_act_dbwd': _flag('accumulate', 'adj_gamma'), 'bn_sync_dbwd_finish': _flag('accumulate', 'adj_gamma'),
    'attn_dbwd_rows': lambda a: ('s', 'gp', 'u', 'v'),           # in place: every output overwrites an input
    'sn_power_iter': lambda a: ('u', 'v'), 'adam_step': lambda a: ('p', 'm', 'v'), 'ema': lambda a: ('t',),
    'center_rows': lambda a: ('X',),
    # channels outside [y_coff, y_coff + C) are neither read nor written: the rest of y must survive
    'inception_conv_fwd': lambda a: ('y',), 'inception_maxpool3s2': lambda a: ('y',), 'inception_avgpool3': lambda a: ('y',),
}

_PARAMS = None


def params_of(name):
    """[(type, argname), ...] of tg_<name> without the trailing stream, from the parsed header."""
    global _PARAMS
    if _PARAMS is None:
        from tartangan_amd import backend
        _PARAMS = backend.parse_header()
    p = _PARAMS['tg_' + name][1]
    return p[:-1] if p and p[-1] == ('void*', 'stream') else p


def _ints(t):
    return t.view(_INT_VIEW.get(t.dtype, t.dtype))


def _pattern(dtype, table):
    return table[dtype] if dtype in table else _INT_PATTERN[dtype]


class _Slot:
    """One tensor placed in the interior of its own guarded buffer."""

    def __init__(self, label, src, role, shift, device, snapshot=False):
        self.label, self.role, self.shift, self.snapshot = label, role, shift, snapshot       # role: 'in' | 'fresh' | 'accum' | 'scratch'
        self.src = src
        n = src.numel()
        self.lo = GUARD + shift
        self.buf = torch.empty(self.lo + n + GUARD, dtype=src.dtype, device=device)
        self.view = self.buf[self.lo:self.lo + n].view(src.shape)
        assert self.view.is_contiguous()
        if shift == 0:
            assert self.view.data_ptr() % 16 == 0, f'{label}: aligned placement is not 16-byte aligned'
        else:
            assert self.view.data_ptr() % 16 == (shift * src.element_size()) % 16
        self.reset()

    def reset(self, finite_guards=False):
        src, ib = self.src, _ints(self.buf)
        if self.role == 'in':
            guard = 0 if finite_guards else (_ints(torch.full((1,), float('nan'), dtype=src.dtype))[0].item()
                                             if src.dtype.is_floating_point else _INT_PATTERN[src.dtype])
        else:
            guard = _pattern(src.dtype, _OUT_SENTINEL)
        ib.fill_(guard)
        if self.role in ('fresh', 'scratch'):
            _ints(self.view).fill_(_pattern(src.dtype, _FRESH_FILL))
        else:
            self.view.copy_(src)
        self.guard_word = guard
        self.before = ib.clone() if self.snapshot else None

    def guard_violation(self):
        ib = _ints(self.buf)
        n = self.src.numel()
        for side, a, b in (('before the start', 0, self.lo), ('past the end', self.lo + n, ib.numel())):
            bad = (ib[a:b] != self.guard_word).nonzero().flatten()
            if bad.numel():
                first, last = int(bad[0]), int(bad[-1])
                off = (lambda i: i - self.lo) if a == 0 else (lambda i: i + 1)       # element offsets from the tensor's edge
                return (f'guard {side} of {self.label} was written: {bad.numel()} element(s), first at offset {off(first)}, '
                        f'last at offset {off(last)} (elements from the {"first" if a == 0 else "last"} element of the tensor)')
        return None

    def unchanged(self):
        return torch.equal(_ints(self.buf), self.before)


def _label(name, i):
    return f'{params_of(name)[i][1]} (argument {i})'


def _roles(name, args, outs, scratch, accum):
    names = [p[1] for p in params_of(name)]
    assert len(names) == len(args), f'{name} takes {len(names)} arguments, got {len(args)}'
    named = dict(zip(names, args))
    rmw = set(accum) | {names.index(n) for n in ACCUM.get(name, lambda a: ())(named) if named[n] is not None}
    assert rmw <= set(outs) | set(scratch), f'{name}: accum {sorted(rmw)} names an argument that is no output'
    roles = {}
    for i, a in enumerate(args):
        if torch.is_tensor(a) or isinstance(a, Per):
            roles[i] = 'accum' if i in rmw else 'scratch' if i in scratch else 'fresh' if i in outs else 'in'
    return roles


def _shift_of(placement, i):
    return 1 if placement == 'shifted' or placement == i else 0


def run_both(K, name, args, outs, tol=1e-5, atol=None, scratch=(), accum=(), placement='aligned', expect='ok', device='cuda',
             emulator=E):
    """args: list of python scalars / CPU tensors / None / HostTable; outs: indices of output tensors; accum: outputs that are
    read-modify-write (on top of ACCUM); placement: 'aligned' | 'shifted' | index of the one pointer argument to shift, or a
    list of those (the emulator runs once for all of them); expect: 'ok' | 'rejected'.
    -> the device-side tensors of the last placement, in argument order (HostTable -> {(row, col): tensor})."""
    scratch = list(scratch) + [i for i, a in enumerate(args) if torch.is_tensor(a) and getattr(a, '_is_ws', False)]
    roles = _roles(name, args, outs, scratch, accum)
    sync = torch.cuda.synchronize if device != 'cpu' else (lambda: None)
    SEEN.add(name)

    def side(a, which):
        return getattr(a, which) if isinstance(a, Per) else a

    # ---- the emulator, once
    cpu, cpu_tab = [], {}
    for i, a in enumerate(args):
        if isinstance(a, HostTable):
            cpu_tab[i] = {pos: side(v, 'emulator').clone() for pos, v in a.cells()}
            cpu.append(a.build(cpu_tab[i]))
        else:
            a = side(a, 'emulator')
            cpu.append(a.clone() if torch.is_tensor(a) else a)
    if expect == 'ok':
        getattr(emulator, name)(*cpu)

    dev = None
    for pl in (placement if isinstance(placement, (list, tuple)) else [placement]):
        assert pl in ('aligned', 'shifted') or (isinstance(pl, int) and pl in roles), f'{name}: placement {pl!r}'
        slots, dev, tabs = {}, [], {}
        for i, a in enumerate(args):
            if isinstance(a, HostTable):
                tabs[i] = {}
                for pos, v in a.cells():
                    role = 'accum' if pos in a.accum else 'scratch' if pos in a.scratch else 'fresh' if pos in a.outs else 'in'
                    s = _Slot(f'{params_of(name)[i][1]}[{pos[0]}][{pos[1]}] (host table)', side(v, 'device'), role,
                              1 if pl == 'shifted' else 0, device, expect == 'rejected')
                    slots[(i, pos)] = s
                    tabs[i][pos] = s.view
                dev.append(a.build(tabs[i]))
            elif i in roles:
                slots[i] = _Slot(_label(name, i), side(a, 'device'), roles[i], _shift_of(pl, i), device, expect == 'rejected')
                dev.append(slots[i].view)
            else:
                dev.append(a)
        where = f'{name} [{pl if isinstance(pl, str) else "only " + _label(name, pl) + " shifted"}]'

        def call():
            getattr(K, name)(*dev)
            sync()

        if expect == 'rejected':
            from tartangan_amd import backend
            try:
                call()
            except backend.KernelError:
                sync()
            else:
                raise AssertionError(f'{where}: accepted a call it documents as unsupported')
            for s in slots.values():
                assert s.unchanged(), f'{where}: rejected the call but wrote {s.label} (or its guards) first'
            continue
        call()
        for s in slots.values():
            v = s.guard_violation()
            assert v is None, f'{where}: {v}'

        def compare(want, got, label, tol, atol):
            want, got = want.double(), got.cpu().double()
            if bool(torch.isnan(got).any()) and not bool(torch.isnan(want).any()):
                at = int(torch.isnan(got).flatten().nonzero()[0])
                # which of the two: run again with finite input guards; a NaN that stays is the output's own fill
                for s in slots.values():
                    s.reset(finite_guards=True)
                call()
                stale = any(bool(torch.isnan(s.view).any()) for s in slots.values() if s.role == 'fresh')
                why = ('depends on its content on entry (declared fresh: elements nobody wrote, or the kernel adds into it)' if stale
                       else 'was reached by a read outside an input (the NaN of an input guard)')
                raise AssertionError(f'{where}: output {label} {why}: NaN at flat index {at} of {got.numel()}')
            scale = float(want.abs().max()) if want.numel() else 1.0
            err = float((want - got).abs().max()) if want.numel() else 0.0
            lim = (atol if atol is not None else tol * max(scale, 1e-6))
            assert err <= lim, f'{where} {label}: max err {err:.3e} > {lim:.3e} (scale {scale:.3e})'

        for i in outs:
            compare(cpu[i], dev[i], f'arg{i} {_label(name, i)}', tol, atol)
        for i, a in enumerate(args):
            if isinstance(a, HostTable):
                for pos in a.outs:
                    compare(cpu_tab[i][pos], tabs[i][pos], slots[(i, pos)].label, a.tol if a.tol is not None else tol, atol)
        for key, s in slots.items():      # inputs must not be modified
            if s.role == 'in':
                assert torch.equal(_ints(s.view.cpu()), _ints(s.src)), f'{where} modified input {key if isinstance(key, int) else ""} {s.label}'
    return [tabs[i] if isinstance(a, HostTable) else d for i, (a, d) in enumerate(zip(args, dev))] if expect == 'ok' else None
