"""Discriminator blocks of the reference (models/blocks/discriminator.py) on HIP kernels.

Implemented: ``DiscriminatorInput`` (discriminator.py:11-22),
``ResidualDiscriminatorBlock`` (:49-95), ``DiscriminatorOutput`` (:126-146),
``IQNDiscriminatorOutput`` (:149-178; ``FusedIQNDiscriminatorOutput``: the same head on one kernel each way),
``MultiModelDiscriminatorOutput`` (:181-201),
``LinearOutput`` (:204-213).  Every op here is differentiable twice
(the real-image branch sits under the R1 penalty).
"""
import functools
import os

import torch
from torch import nn

from ... import functional as TF
from ..iqn import IQN, CosineQuantileEmbedding, iqn_loss
from ..layers import AvgPool2d, BatchNorm2d, Conv2d, LeakyReLU, Linear, Tanh, conv_weight, fusable_conv, interpolate, run_layers

_lrelu = functools.partial(LeakyReLU, 0.2)
_half = functools.partial(interpolate, scale_factor=0.5, mode='bilinear', align_corners=True)


def _is_half(fn):
    """Is ``fn`` the default shortcut resampling?  By value, not identity: a block that went through ``torch.save`` /
    ``torch.load`` or ``copy.deepcopy`` holds its own copy of the partial, and must keep the fused paths below."""
    return fn is _half or (type(fn) is functools.partial and fn.func is _half.func and fn.args == _half.args
                           and fn.keywords == _half.keywords)


class DiscriminatorInput(nn.Module):
    """from-RGB 1x1 convolution"""

    def __init__(self, in_dims, out_dims, conv_factory=Conv2d, activation_factory=_lrelu):
        super().__init__()
        self.convs = nn.Sequential(conv_factory(in_dims, out_dims, 1, padding=0, bias=True))

    def forward(self, img):
        return run_layers(self.convs, img)


class ResidualDiscriminatorBlock(nn.Module):
    """[norm, act,] conv3x3, norm, act, conv3x3, avgpool2  +  bilinear-half(x) [-> conv1x1]"""

    def __init__(self, in_dims, out_dims, first_block=False, norm_factory=BatchNorm2d,
                 conv_factory=Conv2d, avg_pool_factory=AvgPool2d, activation_factory=_lrelu,
                 interpolate=_half):
        super().__init__()
        body = []
        if not first_block:
            body += [norm_factory(in_dims), activation_factory()]
        body += [conv_factory(in_dims, out_dims, 3, padding=1, bias=True),
                 norm_factory(out_dims), activation_factory(),
                 conv_factory(out_dims, out_dims, 3, padding=1, bias=True),
                 avg_pool_factory(2)]
        self.convs = nn.Sequential(*body)
        self.in_dims = in_dims
        self.out_dims = out_dims
        self.project_input = None
        if in_dims != out_dims:
            self.project_input = nn.Sequential(conv_factory(in_dims, out_dims, 1))
        self.interpolate = interpolate

    def forward(self, x):
        if _is_half(self.interpolate):
            shortcut, x = TF.fork_bilinear_half(x)      # one graph node for both uses of x (see functional._ForkBilinearHalf)
        else:
            shortcut = self.interpolate(x)
        if self.project_input is not None:
            shortcut = run_layers(self.project_input, shortcut)
        return run_layers(self.convs, x, residual=shortcut)          # x + h, the add fused into the avg-pool

    def default_resampling(self):
        return _is_half(self.interpolate)

    # ---- the first block fused with the from-RGB 1x1 convolution in front of it
    def fuses_with(self, rgb):
        """True if ``rgb`` (a DiscriminatorInput) followed by this block can run as ``forward_from_rgb``: the block starts
        with a plain 3x3 convolution (first_block: no norm / activation in between), keeps its width and uses the
        default resampling."""
        mods = list(self.convs)
        rc = list(getattr(rgb, 'convs', []))
        return (isinstance(rgb, DiscriminatorInput) and len(rc) == 1 and fusable_conv(rc[0]) and rc[0].kernel_size == (1, 1)
                and rc[0].bias is not None and len(mods) > 1 and fusable_conv(mods[0]) and mods[0].kernel_size == (3, 3)
                and self.project_input is None and _is_half(self.interpolate))

    def forward_from_rgb(self, img, rgb):
        """block(rgb(img)) with the two linear maps in front composed (discriminator.py:11-22 + :60-61: a 1x1 convolution
        directly followed by a 3x3 one).  W'[co][c][tap] = sum_m W3[co][m][tap] W1[m][c]; the from-RGB bias rides on an
        extra all-ones input channel so that zero padding treats it exactly like the reference does at the borders.
        One 4->C 3x3 convolution replaces a 3->C 1x1 and a C->C 3x3 one (C = 16 at 128 px: 4x fewer multiply-adds at
        the full resolution), and the shortcut's bilinear-1/2 runs on the 3-channel image (it commutes with the 1x1)."""
        rgb_conv, conv1 = rgb.convs[0], self.convs[0]
        w1, w3 = conv_weight(rgb_conv), conv_weight(conv1)           # (spectral-norm layers: their effective weights, once per forward)
        C, Cimg = w1.shape[:2]
        Cout = w3.shape[0]
        wc = TF.compose_rgb_filter(w1, rgb_conv.bias, w3)                                             # one launch (and one backwards)
        img_a = img_b = img
        if img.requires_grad and torch.is_grad_enabled():
            img_a, img_b = TF.fork(img, 2)         # two consumers (R1 differentiates w.r.t. the images): one fan-in kernel
        h = TF.conv2d(TF.copy_channels(img_a, Cimg + 1, 1.0), wc.view(Cout, Cimg + 1, 3, 3), conv1.bias)     # [img, 1] in one pass
        if type(rgb_conv) is Conv2d:
            shortcut = run_layers(rgb.convs, self.interpolate(img_b))
        else:
            shortcut = TF.conv2d(self.interpolate(img_b), w1, rgb_conv.bias)
        return run_layers(self.convs[1:], h, residual=shortcut)


class DiscriminatorOutput(nn.Module):
    """norm -> act -> sum over (H, W) -> Linear"""

    def __init__(self, in_dims, out_dims, norm_factory=BatchNorm2d, activation_factory=_lrelu,
                 output_activation_factory=nn.Identity):
        super().__init__()
        self.activation = nn.Sequential(norm_factory(in_dims), activation_factory())
        self.to_output = nn.Sequential(Linear(in_dims, out_dims), output_activation_factory())

    def forward(self, feats):
        feats = run_layers(self.activation, feats)
        # the sum over every dimension behind the channels (discriminator.py:143-144): (H, W), or L for the text trainer
        if TF._is_pair(feats) and feats.r.dim() != 4:
            raise NotImplementedError('DiscriminatorOutput: a Pair of (B, C, L) halves (the shared real | fake pass is 2-D only)')
        feats = TF.sum_tail(feats, 1) if not TF._is_pair(feats) and feats.dim() == 3 else TF.sum_hw(feats)
        return run_layers(self.to_output, feats)


class LinearOutput(nn.Module):
    """Linear -> activation: one head of ``MultiModelDiscriminatorOutput``."""

    def __init__(self, in_dims, out_dims, activation_factory=nn.Identity):
        super().__init__()
        self.xform = nn.Sequential(Linear(in_dims, out_dims), activation_factory())
        self.out_dims = out_dims

    def forward(self, x):
        if self.out_dims == 0:           # (InfoGAN without codes: a head of no columns has nothing to launch)
            if isinstance(x, TF.Pair):
                return TF.Pair(x.r.new_empty(x.r.shape[0], 0), x.f.new_empty(x.f.shape[0], 0))
            return x.new_empty(x.shape[0], 0)
        return run_layers(self.xform, x)


class MultiModelDiscriminatorOutput(nn.Module):
    """norm -> act -> sum over (H, W) -> [head(feats) for head in output_models]: a list, one entry per head.  A ``Pair`` goes
    in, a list of Pairs comes out."""

    def __init__(self, in_dims, out_dims, output_model_factories, norm_factory=BatchNorm2d, activation_factory=_lrelu):
        super().__init__()
        self.activation = nn.Sequential(norm_factory(in_dims), activation_factory())
        self.output_models = nn.ModuleList([factory(in_dims) for factory in output_model_factories])

    def forward(self, feats):
        feats = TF.sum_hw(run_layers(self.activation, feats))
        n = len(self.output_models)
        if not 2 <= n <= 4:
            return [model(feats) for model in self.output_models]
        # The heads' gradients meet at ``feats``: one fan-in kernel instead of the autograd engine's adds.  The halves of a Pair
        # fork separately, so a half that only some heads are differentiated through (the real half's codes are discarded,
        # trainers/info.py:135) sums the gradients that arrive and nobody makes up a zero one for the rest.
        if isinstance(feats, TF.Pair):
            copies = [TF.Pair(r, f) for r, f in zip(TF.fork(feats.r, n), TF.fork(feats.f, n))]
        else:
            copies = TF.fork(feats, n)
        return [model(x) for model, x in zip(self.output_models, copies)]


class IQNDiscriminatorOutput(nn.Module):
    """norm -> act -> sum pool -> IQN quantile mixing -> Linear; returns the quantile
    mean and, when targets are given, the quantile Huber loss."""

    def __init__(self, in_dims, out_dims, norm_factory=BatchNorm2d, activation_factory=_lrelu):
        super().__init__()
        self.activation = nn.Sequential(norm_factory(in_dims), activation_factory())
        self.to_output = nn.Sequential(Linear(in_dims, out_dims))
        self.iqn = IQN(in_dims)
        self.out_dims = out_dims

    def forward(self, feats, targets=None):
        feats = TF.sum_hw(run_layers(self.activation, feats))
        feats_tau, taus = self.iqn(feats)
        p_target_tau = run_layers(self.to_output, feats_tau)
        loss = None
        if targets is not None:
            if self.out_dims != 1:
                raise NotImplementedError('IQN loss kernel covers out_dims == 1 (the trainers\' case)')
            loss = iqn_loss(p_target_tau, targets, taus)
        p_target = TF.mean_reps(p_target_tau, self.iqn.num_quantiles)
        if targets is not None:
            return p_target, loss
        return p_target


class FusedIQNDiscriminatorOutput(IQNDiscriminatorOutput):
    """``IQNDiscriminatorOutput`` whose part behind the pooled features -- embedding, mix, Linear, quantile mean, loss -- is one
    launch each way (``functional.iqn_head``) instead of ~35.  Same constructor, submodules and ``state_dict`` keys; the taus are
    drawn exactly as the composed head draws them (real first, then fake, for a Pair).  BatchNorm -> activation -> sum pool stay
    on their own kernels.  The composed forward of the parent runs instead when the head is not the one the kernel implements
    (``iqn.mix`` other than 'mult', another quantile embedding or activation than cosine + Tanh, more than 20 embedding dims,
    ``out_dims != 1``) or when ``TG_IQN_FUSED_HEAD=0`` is in the environment (read at every call)."""

    def fused(self):
        emb = self.iqn.quantile_embedding
        if os.environ.get('TG_IQN_FUSED_HEAD', '1') == '0' or self.iqn.mix != 'mult' or self.out_dims != 1:
            return False
        if type(emb) is not CosineQuantileEmbedding or len(emb.to_state) != 2 or len(self.to_output) != 1:
            return False
        return (type(emb.to_state[0]) is Linear and type(emb.to_state[1]) is Tanh and type(self.to_output[0]) is Linear
                and emb.to_state[0].bias is not None and self.to_output[0].bias is not None and emb.embedding_dims <= 20)

    def forward(self, feats, targets=None):
        if not self.fused():
            return super().forward(feats, targets=targets)
        feats = TF.sum_hw(run_layers(self.activation, feats))
        if isinstance(feats, TF.Pair):
            batch_size = feats.r.shape[0]
            q_real = self.iqn.sample_quantiles(batch_size)
            taus = TF.Pair(q_real, self.iqn.sample_quantiles(batch_size))
        else:
            taus = self.iqn.sample_quantiles(feats.shape[0])
        emb, out = self.iqn.quantile_embedding, self.to_output[0]
        p_target, loss = TF.iqn_head(feats, taus, targets, emb.to_state[0].weight, emb.to_state[0].bias, out.weight, out.bias,
                                     emb.embedding_range, self.iqn.num_quantiles)
        if targets is not None:
            return p_target, loss
        return p_target
