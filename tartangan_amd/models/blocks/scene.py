"""Scene blocks of the reference (models/blocks/scene.py) on HIP kernels.

Only what trainers.scene instantiates is implemented: ``SceneStructureBlock`` (scene.py:90-160).  Constructor signature,
sub-module names, registration order and initial values follow the reference so state_dicts interchange.
"""
import functools

import torch
from torch import nn

from ... import functional as TF
from ..layers import LeakyReLU, Linear, Sigmoid

_lrelu = functools.partial(LeakyReLU, 0.2)


class SceneStructureBlock(nn.Module):
    """z -> (B, num_patches, scene_size, scene_size): per patch an opacity mask (1 - sigmoid of a Linear of z, or all ones
    without ``refine_patches``), optionally multiplied by one (patch, patch) normal draw shared by the whole batch, placed on
    the canvas by the patch's own affine transform (a second Linear of z).  The reference's Python loop over the patches
    (affine_grid, grid_sample, multiply, squeeze; then stack and permute) is ONE kernel here, ``TF.scene_patches``."""

    def __init__(self, in_dims, num_patches, patch_size=3, scene_size=16, output_orientations=False, refine_patches=False,
                 patch_noise=True, norm_factory=None, activation_factory=_lrelu, **kwargs):
        super().__init__()
        self.patch_area = patch_size ** 2
        # present (and in the state_dict) even when refine_patches is off, like the reference; both Linears draw their default
        # initialisation from the RNG before being overwritten, so a seed gives the reference's initial weights downstream
        self.masks = nn.Sequential(Linear(in_dims, num_patches * self.patch_area), Sigmoid())
        self.masks[0].weight.data.zero_()
        self.masks[0].bias.data.zero_()
        self.patch_transforms = nn.Sequential(Linear(in_dims, 2 * 3 * num_patches))
        self.patch_transforms[0].weight.data.zero_()
        initial_scale = 2
        self.patch_transforms[0].bias.data.copy_(
            torch.tensor([initial_scale, 0, 0, 0, initial_scale, 0], dtype=torch.float).repeat(num_patches))
        self.num_patches = num_patches
        self.output_orientations = output_orientations
        self.scene_size = scene_size
        self.patch_size = patch_size
        self.patch_noise = patch_noise
        if patch_noise:
            self.noise_proto = nn.Parameter(torch.zeros(patch_size, patch_size), requires_grad=False)
        self.refine_patches = refine_patches
        if not refine_patches:
            self.full_masks = nn.Parameter(torch.ones(num_patches, patch_size, patch_size), requires_grad=False)
        self.noise_source = None    # optional callable(rows, cols) -> (rows, cols) device tensor

    def __getstate__(self):
        state = dict(self.__dict__)
        state['noise_source'] = None        # a trainer's hook (bound to its RNG feed): not part of a pickled model
        return state

    def sample_noise(self):
        """One (patch, patch) normal draw per forward, in train and eval mode alike (scene.py:139-140), from the CPU default
        generator and then moved: a seed gives the same noise on any device."""
        if self.noise_source is not None:
            return self.noise_source(self.patch_size, self.patch_size)
        return torch.randn(self.patch_size, self.patch_size).to(self.patch_transforms[0].weight.device)

    def forward(self, z):
        if isinstance(z, TF.Pair):
            raise TypeError('SceneStructureBlock takes one batch of latents, not a Pair (each forward draws its own noise)')
        logits = None
        if self.refine_patches:
            logits = TF.linear(z, self.masks[0].weight, self.masks[0].bias)      # the sigmoid and the `1 -` happen in the kernel
        theta = TF.linear(z, self.patch_transforms[0].weight, self.patch_transforms[0].bias)
        noise = self.sample_noise() if self.patch_noise else None
        return TF.scene_patches(theta, logits, noise, self.patch_size, self.scene_size)

    @property
    def output_channels(self):
        return self.num_patches
