"""Helpers of the InfoGAN trainer's tests (not collected).

* ``InfoEmulator``: ``tests/emulator.Emulator`` plus ``tg_info_code_loss`` computed in float64 from the header's formulas.
* ``code_case``: inputs of one code-loss case, the float64 truth (ATen's ``binary_cross_entropy_with_logits`` / ``mse_loss`` and
  their autograd) and ``e32``, the error the same ATen ops make in float32 on the CPU; ``limit``: the house rule.
* ``info_trainer`` / ``load_info_fixture`` / ``load_procedural``: the trainer a ``tests/golden/info_*.json`` fixture describes."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from emulator import Emulator
from oracle.procedural import procedural_state

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
INFO_CASES = ('info_c16_b4', 'info_c32a2_b4_cat', 'info_c16_b2_id_cont')


# ------------------------------------------------------------------------------------------------------------- emulator
class InfoEmulator(Emulator):
    def info_code_loss(self, codes, z, base, w, out, dcodes, ws, B, C, K, ldz):
        x = codes.reshape(B, C + K).double()
        t = z.reshape(B, ldz)[:, :C + K].double()
        code = torch.zeros((), dtype=torch.float64)
        d = dcodes.view(B, C + K)
        if C:
            xc, tc = x[:, :C], t[:, :C]
            code = code + (xc.clamp(min=0) - xc * tc + torch.log1p(torch.exp(-xc.abs()))).mean()
            d[:, :C] = (w * (torch.sigmoid(xc) - tc) / (B * C)).to(d.dtype)
        if K:
            xk, tk = x[:, C:], t[:, C:]
            code = code + (xk - tk).pow(2).mean()
            d[:, C:] = (w * 2 * (xk - tk) / (B * K)).to(d.dtype)
        o = out.view(-1)
        o[0] = code
        o[1] = (float(base) if base is not None else 0.) + w * code
        return 0


# ----------------------------------------------------------------------------------------------------------- kernel cases
def _rel(got, want):
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / scale if scale > 0 else float((got - want).abs().max())


def limit(e32):
    """The rule of ``shared_cases.limit``: at most 4 x what the same ATen ops are off in fp32 on the same inputs (relative to the
    largest reference value), and never less than 4 fp32 roundoffs."""
    return max(4 * e32, 2.4e-7)


PLANTED = (0., 30., -30., 90., -90.)


@functools.lru_cache(maxsize=None)
def code_case(B, C, K, ldz, w, with_base):
    """One code-loss case, computed once: dict(codes, z, base, want=(out0, out1, dcodes) float64, e32=(three figures)).
    Logits are normal with a few planted at 0, +-30, +-90 (as many as fit); categorical targets are exactly 0 or 1 (a one-hot row);
    the other columns of z are normal."""
    gen = torch.Generator().manual_seed(100000 * B + 1000 * C + 10 * K + ldz)
    codes = torch.randn(B, C + K, generator=gen) * 2
    flat = codes.view(-1)
    where = torch.randperm(flat.numel(), generator=gen)[:len(PLANTED)]
    for i, v in zip(where.tolist(), PLANTED):
        flat[i] = v
    z = torch.randn(B, ldz, generator=gen)
    if C:
        z[:, :C] = 0.
        z[torch.arange(B), torch.randint(0, C, (B,), generator=gen)] = 1.
    base = torch.randn((), generator=gen).abs() + 0.5 if with_base else None

    def both(dtype):
        x = codes.detach().to(dtype).clone().requires_grad_(True)
        t = z.to(dtype)
        code = torch.zeros((), dtype=dtype)
        if C:
            code = code + F.binary_cross_entropy_with_logits(x[:, :C], t[:, :C])
        if K:
            code = code + F.mse_loss(x[:, C:], t[:, C:C + K])
        total = (base.to(dtype) if with_base else 0.) + w * code
        g, = torch.autograd.grad(total, x)
        return code.detach().double().reshape(1), total.detach().double().reshape(1), g.double()
    want, r32 = both(torch.float64), both(torch.float32)
    return dict(codes=codes, z=z, base=base, want=want, e32=tuple(_rel(r, t) for r, t in zip(r32, want)))


# -------------------------------------------------------------------------------------------------------------- fixtures
def load_info_fixture(name):
    with open(os.path.join(GOLDEN_DIR, name + '.json')) as f:
        return json.load(f)


def info_config(fx):
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    return GAN_CONFIGS[fx['config']]._replace(attention=tuple(fx['attention']))


def info_trainer(fx, device, seed=0, cls=None, **overrides):
    from tartangan_amd.trainers.info import InfoTrainer
    cls = cls or InfoTrainer
    tr = cls(cls.default_args(config=info_config(fx), batch_size=fx['batch'], device=device, **{**fx['flags'], **overrides}))
    torch.manual_seed(seed)
    tr.build_models()
    return tr


def load_procedural(tr, fx):
    tr.g.load_state_dict(procedural_state(tr.g.state_dict(), fx['weight_seed']))
    tr.target_g.load_state_dict(procedural_state(tr.target_g.state_dict(), fx['weight_seed'] + 1))
    tr.d.load_state_dict(procedural_state(tr.d.state_dict(), fx['weight_seed'] + 2))


def seed_step_streams(fx):
    torch.manual_seed(fx['rng_seed'])
    np.random.seed(fx['np_seed'])


def total_l2(module, grads=False):
    s = 0.
    for p in module.parameters():
        t = p.grad if grads else p
        if t is not None:
            s += float(t.detach().double().pow(2).sum())
    return s ** 0.5


def step_entry(tr, logs):
    entry = dict(logs)
    entry.update(g_l2=total_l2(tr.g), d_l2=total_l2(tr.d), target_g_l2=total_l2(tr.target_g),
                 g_grad_l2=total_l2(tr.g, True), d_grad_l2=total_l2(tr.d, True))
    return entry
