"""Helpers of the shared-filter trainer's tests (not collected).

* ``SharedEmulator``: ``tests/emulator.Emulator`` plus the four entry points of the shared family in plain torch
  (``tg_bilinear_up2x_fwd`` / ``_bwd`` through ``F.interpolate`` and its autograd, ``tg_filter_narrow`` / ``_bwd`` by slicing).
* ``up_case``: inputs of one bilinear x2 case, the float64 truth of forward and transpose, and ``e32``, the error the same ATen
  op makes in float32 on the CPU.
* ``shared_state``: procedural weights for a shared-filter state_dict (``oracle.procedural`` has no rule for the bank).
* ``shared_trainer`` / ``load_shared_fixture``: the trainer a ``tests/golden/shared_*.json`` fixture describes."""
import functools
import json
import os

import torch
import torch.nn.functional as F

from emulator import Emulator
from oracle.procedural import procedural_state

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SHARED_CASES = ('shared_c16_b4', 'shared_c32a2_b4', 'shared_c64_b2_id')


def up(x):
    return F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True)


def up_transpose(gy, dtype=None):
    """(1, BC, 2H, 2W) -> (1, BC, H, W): the transpose of ``up`` through ATen's own backward, in ``dtype`` (default: gy's)."""
    dtype = dtype or gy.dtype
    with torch.enable_grad():
        xin = torch.zeros(gy.shape[0], gy.shape[1], gy.shape[2] // 2, gy.shape[3] // 2, dtype=dtype, requires_grad=True)
        g, = torch.autograd.grad(up(xin), xin, gy.detach().to(dtype))
    return g


# ------------------------------------------------------------------------------------------------------------- emulator
class SharedEmulator(Emulator):
    def bilinear_up2x_fwd(self, x, residual, y, BC, H, W):
        r = up(x.reshape(1, BC, H, W))[0]
        y.copy_((r if residual is None else residual.reshape(BC, 2 * H, 2 * W) + r).reshape(y.shape))
        return 0

    def bilinear_up2x_bwd(self, gy, residual, gx, BC, H, W):
        g = up_transpose(gy.reshape(1, BC, 2 * H, 2 * W))[0]
        gx.copy_((g if residual is None else residual.reshape(BC, H, W) + g).reshape(gx.shape))
        return 0

    def filter_narrow(self, bank, view, O, I, Omax, Imax, taps):
        view.copy_(bank.reshape(Omax, Imax, taps)[:O, :I].reshape(view.shape))
        return 0

    def filter_narrow_bwd(self, gview, gbank, O, I, Omax, Imax, taps, accumulate):
        b = gbank.view(Omax, Imax, taps)
        if not accumulate:
            b.zero_()
        b[:O, :I] += gview.reshape(O, I, taps)
        return 0


# ----------------------------------------------------------------------------------------------------------- kernel cases
def _rel(got, want):
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / scale if scale > 0 else float((got - want).abs().max())


@functools.lru_cache(maxsize=None)
def up_case(BC, H, W, residual):
    """One bilinear x2 case, computed once: dict(x, gy, res_y, res_x, want=(y, gx) float64, e32=(fwd, bwd))."""
    gen = torch.Generator().manual_seed(1000 * BC + 10 * H + W)
    x, gy = torch.randn(BC, H, W, generator=gen), torch.randn(BC, 2 * H, 2 * W, generator=gen)
    res_y = torch.randn(BC, 2 * H, 2 * W, generator=gen) if residual else None
    res_x = torch.randn(BC, H, W, generator=gen) if residual else None

    def both(dtype):
        y = up(x.to(dtype)[None])[0]
        g = up_transpose(gy[None], dtype)[0]
        if residual:
            y, g = res_y.to(dtype) + y, res_x.to(dtype) + g
        return y.double(), g.double()
    want, r32 = both(torch.float64), both(torch.float32)
    return dict(x=x, gy=gy, res_y=res_y, res_x=res_x, want=want, e32=tuple(_rel(r, w) for r, w in zip(r32, want)))


def limit(e32):
    """The rule of ``scene_cases.limit``: at most 4 x what the same ATen op is off in fp32 on the same inputs (relative to the
    largest reference value), and never less than 4 fp32 roundoffs."""
    return max(4 * e32, 2.4e-7)


# --------------------------------------------------------------------------------------------------------------- weights
def shared_state(template, seed):
    """Procedural weights for a SharedGenerator / SharedDiscriminator state_dict.  ``oracle.procedural.procedural_state`` has no
    rule for ``shared_filters``; the bank gets N(0, 1.6 / fan_in) with the fan-in of the whole bank (Imax * 9), drawn once, and
    every alias key (``blocks.1.shared_filters``, ``blocks.1.blocks.0.shared_filters``, ...) carries that same value."""
    rest = {k: v for k, v in template.items() if k.rsplit('.', 1)[-1] != 'shared_filters'}
    state = procedural_state(rest, seed)
    bank = template['shared_filters']
    gen = torch.Generator().manual_seed(seed * 7919 + 101)
    value = torch.randn(bank.shape, generator=gen) * (1.6 / bank[0].numel()) ** 0.5
    for k in template:
        if k not in rest:
            state[k] = value.clone()
    return {k: state[k] for k in template}


# -------------------------------------------------------------------------------------------------------------- fixtures
def load_shared_fixture(name):
    with open(os.path.join(GOLDEN_DIR, name + '.json')) as f:
        return json.load(f)


def shared_config(fx):
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    return GAN_CONFIGS[fx['config']]._replace(attention=tuple(fx['attention']))


def shared_trainer(fx, device, seed=0, **overrides):
    from tartangan_amd.trainers.shared.cnn import CNNTrainer
    tr = CNNTrainer(CNNTrainer.default_args(config=shared_config(fx), batch_size=fx['batch'], device=device, **fx['flags'],
                                            **overrides))
    torch.manual_seed(seed)
    tr.build_models()
    return tr


def load_procedural(tr, fx):
    tr.g.load_state_dict(shared_state(tr.g.state_dict(), fx['weight_seed']))
    tr.target_g.load_state_dict(shared_state(tr.target_g.state_dict(), fx['weight_seed'] + 1))
    tr.d.load_state_dict(shared_state(tr.d.state_dict(), fx['weight_seed'] + 2))
