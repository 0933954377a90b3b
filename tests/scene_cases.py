"""Helpers of the scene-trainer tests (not collected).

* ``compose``: the reference's own formulation of the structure stage (models/blocks/scene.py:127-155) -- a loop over the
  patches of ``F.affine_grid`` + ``F.grid_sample`` -- in a chosen dtype, with autograd for the backward.
* ``SceneEmulator``: ``tests/emulator.Emulator`` plus ``tg_scene_patches_fwd`` / ``_bwd`` computed from it in float64.
* ``kernel_case``: inputs of one kernel case, the float64 truth and ``e32``, the error plain fp32 ATen makes on them.
* ``scene_state``: procedural weights for a ``StructuredSceneGenerator`` state_dict.
* ``scene_trainer`` / ``load_scene_fixture``: the trainer a ``tests/golden/scene_*.json`` fixture describes."""
import functools
import json
import os

import torch
import torch.nn.functional as F

from emulator import Emulator
from oracle.procedural import procedural_state

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SCENE_CASES = ('scene_c32_s8_p5_b4', 'scene_c64_s16_p20_b4_refine_noise', 'scene_c32_s4_p3_k4_b4_refine')
INIT_THETA = (2., 0., 0., 0., 2., 0.)
KINK_MARGIN = 1e-4          # least distance of a sample coordinate from an integer texel coordinate (float64)


# ------------------------------------------------------------------------------------------------------ the restatement
def compose(theta, mask_logits, noise, B, P, patch, S):
    """(B, P, S, S) in the dtype of ``theta``; differentiable."""
    transforms = theta.view(B, P, 2, 3)
    if mask_logits is not None:
        masks = (1. - torch.sigmoid(mask_logits)).view(B, P, patch, patch)
    else:
        masks = torch.ones(B, P, patch, patch, dtype=theta.dtype)
    planes = []
    for i in range(P):
        mask = masks[:, i][:, None]
        if noise is not None:
            mask = mask * noise
        grid = F.affine_grid(transforms[:, i], (B, 1, S, S), align_corners=False)
        planes.append(F.grid_sample(mask, grid, mode='bilinear', padding_mode='zeros', align_corners=False).squeeze(1))
    return torch.stack(planes, dim=0).permute(1, 0, 2, 3)


def compose_both(theta, mask_logits, noise, gout, B, P, patch, S, dtype):
    """-> (out, gtheta, gmask_logits or None) of the composition run in ``dtype``, as float64."""
    th = theta.detach().to(dtype).clone().requires_grad_(True)
    lg = mask_logits.detach().to(dtype).clone().requires_grad_(True) if mask_logits is not None else None
    nz = noise.detach().to(dtype) if noise is not None else None
    out = compose(th, lg, nz, B, P, patch, S)
    grads = torch.autograd.grad(out, [th] + ([lg] if lg is not None else []), gout.to(dtype).view(B, P, S, S))
    return out.detach().double(), grads[0].double(), (grads[1].double() if lg is not None else None)


def sample_coordinates(theta, B, P, patch, S):
    """Texel coordinates (ix, iy), each (B, P, S, S), of every sample, in float64."""
    th = theta.double().view(B, P, 2, 3)
    base = (2 * torch.arange(S, dtype=torch.float64) + 1) / S - 1
    x, y = base.view(1, 1, 1, S), base.view(1, 1, S, 1)
    gx = th[:, :, 0, 0, None, None] * x + th[:, :, 0, 1, None, None] * y + th[:, :, 0, 2, None, None]
    gy = th[:, :, 1, 0, None, None] * x + th[:, :, 1, 1, None, None] * y + th[:, :, 1, 2, None, None]
    return ((gx + 1) * patch - 1) / 2, ((gy + 1) * patch - 1) / 2


def kink_distance_and_coverage(theta, B, P, patch, S):
    """-> (least distance to an integer over the coordinates of every sample that can reach the patch, share of the samples
    inside the patch).  A sample reaches the patch when both coordinates lie in (-1, patch); the distance is taken over a band
    half a texel wider on each side, so a sample within rounding of the patch's outer edge counts too."""
    ix, iy = sample_coordinates(theta, B, P, patch, S)
    inside = (ix > -1) & (ix < patch) & (iy > -1) & (iy < patch)
    near = (ix > -1.5) & (ix < patch + 0.5) & (iy > -1.5) & (iy < patch + 0.5)
    coords = torch.cat([ix[near], iy[near]])
    dist = float((coords - coords.round()).abs().min()) if coords.numel() else 1.0
    return dist, float(inside.double().mean())


# ------------------------------------------------------------------------------------------------------------- emulator
class SceneEmulator(Emulator):
    def scene_patches_fwd(self, theta, mask_logits, noise, out, B, P, patch, S):
        with torch.no_grad():
            r = compose(theta.double(), mask_logits.double() if mask_logits is not None else None,
                        noise.double() if noise is not None else None, B, P, patch, S)
        out.copy_(r.reshape(out.shape))
        return 0

    def scene_patches_bwd(self, gout, theta, mask_logits, noise, gtheta, gmask_logits, B, P, patch, S):
        assert (mask_logits is None) == (gmask_logits is None)
        with torch.enable_grad():
            _, gt, gm = compose_both(theta, mask_logits, noise, gout, B, P, patch, S, torch.float64)
        gtheta.copy_(gt.reshape(gtheta.shape))
        if gmask_logits is not None:
            gmask_logits.copy_(gm.reshape(gmask_logits.shape))
        return 0


# ----------------------------------------------------------------------------------------------------------- kernel cases
def _inputs(B, P, patch, S, seed):
    gen = torch.Generator().manual_seed(seed)
    theta = torch.tensor(INIT_THETA).repeat(B, P) + 0.6 * torch.randn(B, P * 6, generator=gen)
    logits = torch.randn(B, P * patch * patch, generator=gen)
    noise = torch.randn(patch, patch, generator=gen)
    gout = torch.randn(B, P, S, S, generator=gen)
    return theta.contiguous(), logits, noise, gout


def _rel(got, want):
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / scale if scale > 0 else float((got - want).abs().max())


@functools.lru_cache(maxsize=None)
def kernel_case(B, P, patch, S, masks=True, noise=True, theta='random'):
    """One kernel case, computed once: dict(theta, logits, noise, gout, seed, dist, coverage, want=(out, gtheta, gmask),
    e32=(...)).  theta 'random': the init pattern + 0.6 randn, from the first seed in 0..199 under which (float64) every
    coordinate of a sample that can reach the patch is at least 1e-4 from an integer and 20 % .. 90 % of the samples fall inside
    the patch; 'init': the exact init pattern; 'off': every patch translated off the canvas."""
    if theta == 'random':
        for seed in range(200):
            th, lg, nz, go = _inputs(B, P, patch, S, seed)
            dist, cov = kink_distance_and_coverage(th, B, P, patch, S)
            if dist >= KINK_MARGIN and 0.2 <= cov <= 0.9:
                break
        else:
            raise AssertionError(f'no seed in 0..199 gives a usable case for {(B, P, patch, S)}')
    else:
        seed = 0
        _, lg, nz, go = _inputs(B, P, patch, S, seed)
        th = torch.tensor(INIT_THETA if theta == 'init' else (2., 0., 50., 0., 2., -50.)).repeat(B, P).contiguous()
        dist, cov = kink_distance_and_coverage(th, B, P, patch, S)
        assert dist >= KINK_MARGIN
    lg, nz = (lg if masks else None), (nz if noise else None)
    want = compose_both(th, lg, nz, go, B, P, patch, S, torch.float64)
    r32 = compose_both(th, lg, nz, go, B, P, patch, S, torch.float32)
    e32 = tuple(None if w is None else _rel(r, w) for r, w in zip(r32, want))
    return dict(theta=th, logits=lg, noise=nz, gout=go, seed=seed, dist=dist, coverage=cov, want=want, e32=e32)


def limit(e32):
    """The most the kernel may be off (relative to the largest reference value): 4 x what plain fp32 ATen is off on the same
    inputs -- another summation order over S*S terms, another sigmoid evaluation -- and never less than 4 fp32 roundoffs."""
    return max(4 * e32, 2.4e-7)


# --------------------------------------------------------------------------------------------------------------- weights
def scene_state(template, seed):
    """Procedural weights for a StructuredSceneGenerator state_dict.  ``oracle.procedural.procedural_state`` has no rule for
    ``full_masks`` / ``noise_proto`` (kept as they are) and would give the two names of the structure block's tensors
    (``structure_generator.X`` and ``blocks.0.X``) different values (``blocks.0.X`` takes ``structure_generator.X``'s).  The
    transform bias is the init pattern plus the procedural perturbation."""
    keep = {k: v.clone() for k, v in template.items() if k.rsplit('.', 1)[-1] in ('full_masks', 'noise_proto')}
    state = procedural_state({k: v for k, v in template.items() if k not in keep}, seed)
    state.update(keep)
    key = 'structure_generator.patch_transforms.0.bias'
    state[key] = state[key] + torch.tensor(INIT_THETA).repeat(state[key].numel() // 6)
    for k in list(state):
        if k.startswith('structure_generator.'):
            state['blocks.0.' + k[len('structure_generator.'):]] = state[k].clone()
    return {k: state[k] for k in template}


# -------------------------------------------------------------------------------------------------------------- fixtures
def load_scene_fixture(name):
    with open(os.path.join(GOLDEN_DIR, name + '.json')) as f:
        return json.load(f)


def scene_trainer(fx, device, seed=0):
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    from tartangan_amd.trainers.scene import SceneTrainer
    tr = SceneTrainer(SceneTrainer.default_args(config=GAN_CONFIGS[fx['config']], batch_size=fx['batch'], device=device,
                                                **fx['flags']))
    torch.manual_seed(seed)
    tr.build_models()
    return tr


def load_procedural(tr, fx):
    tr.g.load_state_dict(scene_state(tr.g.state_dict(), fx['weight_seed']))
    tr.target_g.load_state_dict(scene_state(tr.target_g.state_dict(), fx['weight_seed'] + 1))
    tr.d.load_state_dict(procedural_state(tr.d.state_dict(), fx['weight_seed'] + 2))
