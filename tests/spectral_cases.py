"""Helpers of the batched spectral-norm tests (not collected).

* ``SpectralEmulator``: ``tests/emulator.Emulator`` plus float64 forms (rounded to the output's dtype) of tg_sn_batch_workspace /
  tg_sn_batch_fwd / tg_sn_batch_bwd, written from the header's formulas.
* ``reference_fwd`` / ``reference_bwd``: the same quantities from plain torch ops (``F.normalize``, ``mv``, ``dot`` and autograd
  through ``W / dot(u, W v)``) in a given dtype: float64 is the truth, float32 on the CPU gives ``e32``.
* ``make_layers`` / ``table``: the matrices of the kernel tests and their host item table.
* ``limit`` / ``rel``: the house rule of DESIGN §5."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from emulator import Emulator

FIELDS = 8
# what the kernels tile by (csrc/spectral.hip): rows per W^T u slab, columns per W^T u chunk, flat elements per element-wise chunk
SN_SLAB, SN_COLS, SN_ELEMS = 64, 256, 2048
# rows x cols: the to-RGB 1x1, D's first 3x3, a 1x1, ragged in both axes (two row slabs with a ragged last one, two column chunks
# with a ragged tail, cols % 4 != 0), and the two largest filters of the benchmarked configs
SHAPES = [(3, 16), (16, 27), (64, 64), (70, 333), (128, 1152), (256, 2304)]


def limit(e32):
    """At most 4 x what the same ATen ops are off in fp32 on the same inputs (relative to the largest reference value), and
    never less than 4 fp32 roundoffs."""
    return max(4 * e32, 2.4e-7)


def rel(got, want):
    scale = float(want.abs().max())
    err = float((got.double() - want.double()).abs().max())
    return err / scale if scale > 0 else err


def _at(addr, n):          # a float32 view of host memory (every tensor is a CPU tensor under the emulator)
    return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(addr)))


def reference_fwd(W, u, v, update, eps, dtype):
    """-> u', v', sigma, w_sn with torch's ops in ``dtype`` (torch.nn.utils.spectral_norm's compute_weight, one iteration)."""
    W, u, v = W.to(dtype), u.to(dtype), v.to(dtype)
    if update:
        v = F.normalize(torch.mv(W.t(), u), dim=0, eps=eps)
        u = F.normalize(torch.mv(W, v), dim=0, eps=eps)
    sigma = torch.dot(u, torch.mv(W, v))
    return u, v, sigma, W / sigma


def reference_bwd(W, u, v, g_sn, dtype):
    """-> d<g_sn, W / sigma(W)>/dW by autograd, u and v constants."""
    W = W.to(dtype).clone().requires_grad_(True)
    u, v = u.to(dtype), v.to(dtype)
    with torch.enable_grad():
        w_sn = W / torch.dot(u, torch.mv(W, v))
        g, = torch.autograd.grad((w_sn * g_sn.to(dtype)).sum(), W)
    return g


def bwd_formula(g_sn, w_sn, u, v, sigma, dtype):
    """(g_sn - <g_sn, w_sn> u v^T) / sigma in ``dtype``: the header's formula on exactly what tg_sn_batch_bwd is handed."""
    g, w = g_sn.to(dtype), w_sn.to(dtype)
    d = torch.dot(g.reshape(-1), w.reshape(-1))
    return (g - d * torch.outer(u.to(dtype), v.to(dtype))) / sigma.to(dtype)


class SpectralEmulator(Emulator):
    def _rows(self, items, n_items):
        assert items.dtype == torch.int64 and tuple(items.shape) == (n_items, FIELDS)
        return items.tolist()

    def sn_batch_workspace(self, items, n_items):
        if items is None or n_items < 1:
            return 0
        return 16 * n_items

    def sn_batch_fwd(self, items, n_items, sigma, workspace, workspace_bytes, update, eps):
        assert workspace_bytes >= self.sn_batch_workspace(items, n_items)
        for i, (w, u, v, wsn, _, _, rows, cols) in enumerate(self._rows(items, n_items)):
            W, ut, vt = _at(w, rows * cols).view(rows, cols), _at(u, rows), _at(v, cols)
            un, vn, s, out = reference_fwd(W, ut, vt, update, eps, torch.float64)
            if update:
                ut.copy_(un.float())
                vt.copy_(vn.float())
            sigma[i] = s.float()
            _at(wsn, rows * cols).copy_(out.float().reshape(-1))
        return 0

    def sn_batch_bwd(self, items, n_items, sigma, workspace, workspace_bytes, clear):
        assert workspace_bytes >= self.sn_batch_workspace(items, n_items)
        for i, (_, u, v, wsn, gsn, gorig, rows, cols) in enumerate(self._rows(items, n_items)):
            n = rows * cols
            g, w_sn = _at(gsn, n), _at(wsn, n).double()
            d = torch.dot(g.double(), w_sn)
            r = (g.double().view(rows, cols) - d * torch.outer(_at(u, rows).double(), _at(v, cols).double())) / float(sigma[i])
            dst = _at(gorig, n)
            dst.copy_((dst.double() + r.reshape(-1)).float())
            if clear:
                g.zero_()
        return 0


EMU = SpectralEmulator()


def make_layers(shapes=SHAPES, seed=0):
    """Per matrix: W ~ N(0, 1/cols), unit u and v, an upstream gradient g_sn and a non-zero g_orig to accumulate into."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for rows, cols in shapes:
        W = torch.randn(rows, cols, generator=g) / cols ** 0.5
        u = F.normalize(torch.randn(rows, generator=g), dim=0)
        v = F.normalize(torch.randn(cols, generator=g), dim=0)
        out.append(dict(W=W, u=u, v=v, g_sn=torch.randn(rows, cols, generator=g), g_orig=torch.randn(rows, cols, generator=g),
                        rows=rows, cols=cols))
    return out


def low_rank(rows, cols, seed=0):
    """W = 3 a b^T + 0.1 N(0, 1/cols): a dominant singular value the power iteration reaches in a few steps."""
    g = torch.Generator().manual_seed(seed)
    a = F.normalize(torch.randn(rows, generator=g, dtype=torch.float64), dim=0)
    b = F.normalize(torch.randn(cols, generator=g, dtype=torch.float64), dim=0)
    return (3 * torch.outer(a, b) + 0.1 * torch.randn(rows, cols, generator=g, dtype=torch.float64) / cols ** 0.5).float()
