"""Shared-filter blocks of the reference (models/shared/blocks.py) on HIP kernels.

Every 3x3 convolution of a network -- the shortcut projections included, which here are unbiased 3x3 convolutions and not
1x1 -- reads the leading ``[out_dims, in_dims]`` corner of ONE parameter, ``shared_filters[Omax, Imax, 3, 3]``
(``narrow_filters``).  The generator block upsamples x2 bilinearly (align_corners=True) in front of its convolutions, the
discriminator block halves both its main path and its shortcut bilinearly.  Constructor signatures, sub-module names and
registration order follow the reference so state_dicts interchange: the bank appears under every alias
(``blocks.1.shared_filters``, ``blocks.1.blocks.0.shared_filters``, ...), ``named_parameters()`` lists it once.  Like the
reference, a block with ``apply_norm=False`` still owns its ``norm_and_activate`` (BatchNorm parameters that never receive a
gradient).  Every forward accepts a ``functional.Pair``.
"""
import functools

import torch
from torch import nn

from ... import functional as TF
from ..layers import BatchNorm2d, LeakyReLU, run_layers

_lrelu = functools.partial(LeakyReLU, 0.2)


def narrow_filters(filters, in_dims, out_dims):
    """Extract the first NxM filters (reference blocks.py:124-127), as the dense tensor the convolution kernels take."""
    return TF.narrow_filters(filters, in_dims, out_dims)


class SharedConvBlock(nn.Module):
    """[norm, act,] conv3x3 with the bank's (out_dims, in_dims) corner, own bias (blocks.py:8-40)."""

    def __init__(self, shared_filters, in_dims, out_dims, apply_norm=True, bias=True,
                 norm_factory=BatchNorm2d, activation_factory=_lrelu):
        super().__init__()
        self.norm_and_activate = nn.Sequential(norm_factory(in_dims), activation_factory())
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_dims, requires_grad=True))
        else:
            self.bias = None
        self.shared_filters = shared_filters
        self.in_dims = in_dims
        self.out_dims = out_dims
        self.apply_norm = apply_norm

    def forward(self, x, residual=None):
        """``residual``: the block's shortcut, added in the convolution's epilogue."""
        if self.apply_norm:
            x = run_layers(self.norm_and_activate, x)
        return TF.conv2d(x, narrow_filters(self.shared_filters, self.in_dims, self.out_dims), self.bias, residual)


class _SharedResidualBlock(nn.Module):
    def __init__(self, shared_filters, in_dims, out_dims, apply_norm=True, bias=True,
                 norm_factory=BatchNorm2d, activation_factory=_lrelu):
        super().__init__()
        self.blocks = nn.Sequential(
            SharedConvBlock(shared_filters, in_dims, out_dims, apply_norm=apply_norm, bias=bias,
                            norm_factory=norm_factory, activation_factory=activation_factory),
            SharedConvBlock(shared_filters, out_dims, out_dims, apply_norm=True, bias=bias,
                            norm_factory=norm_factory, activation_factory=activation_factory),
        )
        self.shared_filters = shared_filters
        self.in_dims = in_dims
        self.out_dims = out_dims

    def project_input(self, x, residual=None):
        """unbiased 3x3 convolution with the bank's (out_dims, in_dims) corner [+ residual]"""
        return TF.conv2d(x, narrow_filters(self.shared_filters, self.in_dims, self.out_dims), None, residual)


class SharedResidualGeneratorBlock(_SharedResidualBlock):
    """x = up(x); h = blocks(x); return (project_input(x) if the width changes else x) + h   (blocks.py:43-78)"""

    def forward(self, x):
        xs, xu = TF.fork_bilinear_up2x(x)          # one graph node for both uses of the upsampled input
        shortcut = xs if self.in_dims == self.out_dims else self.project_input(xs)
        first, last = self.blocks
        return last(first(xu), residual=shortcut)  # x + h, the add in the last convolution's epilogue


class SharedResidualDiscriminatorBlock(_SharedResidualBlock):
    """h = half(blocks(x)); x = half(x); return (project_input(x) if the width changes else x) + h   (blocks.py:81-121)"""

    def forward(self, x):
        shortcut, x = TF.fork_bilinear_half(x)     # one graph node for both uses of x
        first, last = self.blocks
        h = TF.bilinear_half(last(first(x)))
        if self.in_dims != self.out_dims:
            return self.project_input(shortcut, residual=h)      # x + h, the add in the projection's epilogue
        return TF.add(shortcut, h)
