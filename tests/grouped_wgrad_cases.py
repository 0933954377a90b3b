"""Shared by tests/test_grouped_wgrad.py (CPU) and tests/test_grouped_wgrad_gpu.py: the emulator with the grouped stage 1 of the
1x1 weight gradients (tg_conv1x1_wgrad_partials_batch) and the shapes of its cases.  TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np
import torch

from emulator import Emulator

FIELDS = 15          # TG_WGRAD1X1_ITEM_FIELDS


def _at(addr, n):
    """A float32 view of host memory (every tensor is a CPU tensor under the emulator)."""
    return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(addr)))


class GroupedEmulator(Emulator):
    """The emulator plus the batch entry as a loop over ``conv2d_wgrad_partials`` (three gy tensors: their concatenation)."""

    def conv1x1_wgrad_batch_supported(self, B, Cin, Cout, H, W):
        return int((H * W) % 16 == 0)

    def conv1x1_wgrad_partials_batch(self, items, n_items):
        assert items.dtype == torch.int64 and tuple(items.shape) == (n_items, FIELDS)
        for x, gy0, gy1, gy2, ws, ws_bytes, c0, c1, c2, B, Cin, H, W, ks, want_bias in items.tolist():
            assert ks == 1 and (H * W) % 16 == 0 and c0 > 0 and (c1 > 0) == (c2 > 0) == bool(gy1) == bool(gy2)
            assert all(p % 16 == 0 for p in (x, gy0, gy1, gy2, ws))
            gy = torch.cat([_at(p, B * c * H * W).view(B, c, H, W) for p, c in ((gy0, c0), (gy1, c1), (gy2, c2)) if c], 1).contiguous()
            self.conv2d_wgrad_partials(_at(x, B * Cin * H * W), gy, _at(ws, ws_bytes // 4), ws_bytes, B, Cin, c0 + c1 + c2, H, W, 1, want_bias)
        return 0


# (B, Cin, (c0[, c1, c2]), H, W, bias): the smallest shapes that reach each path of the grouped kernel
CASES = {
    'a': (1, 16, (16,), 4, 4, False),            # one 16-pixel group, S = 1, three waves with empty ranges
    'b': (2, 3, (16,), 8, 8, False),             # clamped input rows, <1, 1>
    'c': (1, 16, (3,), 16, 16, True),            # clamped output rows, bias partials
    'd': (2, 32, (64,), 8, 8, True),             # <2, 2>
    'e': (3, 64, (128,), 4, 4, False),           # 4 x 2 channel tiles over three pixel groups: S smaller than the tile grid suggests
    'f': (2, 32, (4, 4, 16), 8, 8, False),       # theta | phi | g: three gy tensors
}
