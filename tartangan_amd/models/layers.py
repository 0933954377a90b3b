"""HIP-backed layer modules.

The reference's ``models/layers.py:6-22`` holds ``Interpolate`` and
``PixelNorm``; the reference blocks otherwise take stock ``torch.nn`` layers
through their ``norm_factory`` / ``conv_factory`` / ``activation_factory`` /
``avg_pool_factory`` hooks (models/blocks/discriminator.py:50-58,
generator.py:33-35).  The classes here are what this package plugs into those
hooks: same constructor signatures, same parameters / buffers / state_dict
keys and the same default initialisation (they subclass the torch modules and
only replace ``forward``), but the arithmetic runs in libtartangan_amd.so.
"""
import functools

import torch
from torch import nn

from .. import functional as TF


class Conv2d(nn.Conv2d):
    """nn.Conv2d restricted to what the hot path uses: 3x3/pad 1 or 1x1/pad 0, stride 1."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, bias=True, **kw):
        super().__init__(in_channels, out_channels, kernel_size, padding=padding, bias=bias, **kw)
        ks = self.kernel_size
        ok = (ks in ((1, 1), (3, 3)) and self.padding == (ks[0] // 2, ks[0] // 2)
              and self.stride == (1, 1) and self.dilation == (1, 1) and self.groups == 1)
        if not ok:
            raise ValueError(f'tartangan_amd.Conv2d supports 3x3/pad1 and 1x1/pad0 stride-1 only, got {self}')

    def forward(self, x):
        return TF.conv2d(x, self.weight, self.bias)


class SpectralNormConv2d(Conv2d):
    """``conv_factory`` with spectral normalisation (what ``torch.nn.utils.spectral_norm(nn.Conv2d(...))`` gives):
    parameters ``weight_orig`` / ``bias``, buffers ``weight_u`` / ``weight_v``, one power iteration per training
    forward, ``weight = weight_orig / sigma``.  Off by default: the reference's trainers never apply it.

    Inside a ``functional.spectral_scope`` opened for a network that holds the layer (the trainers' ``--spectral-norm``), the
    weight is the one the scope materialised for all of the network's layers at once: no iteration per forward, the same
    weight for every forward of the scope, its gradient mapped back by ``functional.spectral_backward``."""

    def __init__(self, *args, n_power_iterations=1, eps=1e-12, **kw):
        super().__init__(*args, **kw)
        weight = self._parameters.pop('weight')
        self.register_parameter('weight_orig', weight)
        with torch.no_grad():
            h, w = weight.shape[0], weight[0].numel()
            u = nn.functional.normalize(weight.new_empty(h).normal_(0, 1), dim=0, eps=eps)
            v = nn.functional.normalize(weight.new_empty(w).normal_(0, 1), dim=0, eps=eps)
        self.register_buffer('weight_u', u)
        self.register_buffer('weight_v', v)
        self.n_power_iterations, self.sn_eps = n_power_iterations, eps

    _sn_leaf = None          # set by an open functional.spectral_scope: the materialised weight_orig / sigma (a leaf)

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_sn_leaf', None)            # a view of a scope's arena does not travel with a checkpoint
        return state

    def effective_weight(self):
        """The filter this forward convolves with.  Outside a spectral scope: one power iteration now (training mode), then
        ``weight_orig / sigma`` differentiable w.r.t. ``weight_orig`` -- call it ONCE per forward."""
        leaf = self._sn_leaf
        if leaf is not None:
            if leaf.requires_grad != self.weight_orig.requires_grad:        # (toggle_grad only reaches parameters)
                leaf.requires_grad_(self.weight_orig.requires_grad)
            return leaf
        return TF.spectral_normalize(self.weight_orig, self.weight_u, self.weight_v, self.training,
                                     self.n_power_iterations, self.sn_eps)

    def forward(self, x):
        return TF.conv2d(x, self.effective_weight(), self.bias)


def fusable_conv(m):
    """A convolution layer whose filter ``run_layers`` and the blocks may hand to a fused route themselves."""
    return type(m) is Conv2d or type(m) is SpectralNormConv2d


def conv_weight(m):
    """The filter of a ``fusable_conv`` layer (a spectral-norm layer: see ``effective_weight``, once per forward)."""
    return m.weight if type(m) is Conv2d else m.effective_weight()


def strip_spectral_norm(state_dict):
    """A plain state_dict from one with spectral-norm layers (the role of ``remove_all_spectral_norm`` in the reference's
    prep4web.py:33-51): every ``X.weight_orig`` / ``X.weight_u`` / ``X.weight_v`` triple becomes ``X.weight = weight_orig /
    sigma`` with ``sigma = u^T W v`` from the stored u and v (no iteration: what the layer computes in eval mode).  Other keys
    pass through; the order of the keys is kept.  A stock ``Generator`` / ``Discriminator`` loads the result."""
    out = type(state_dict)()
    for key, val in state_dict.items():
        if key.endswith('weight_u') or key.endswith('weight_v'):
            continue
        if key.endswith('weight_orig'):
            stem = key[:-len('_orig')]
            u, v = state_dict[stem + '_u'].double(), state_dict[stem + '_v'].double()
            w = val.detach().double()
            sigma = torch.dot(u, torch.mv(w.reshape(w.shape[0], -1), v))
            out[stem] = (w / sigma).to(val.dtype)
        else:
            out[key] = val
    meta = getattr(state_dict, '_metadata', None)
    if meta is not None:
        out._metadata = meta
    return out


class Linear(nn.Linear):
    def forward(self, x):
        return TF.linear(x, self.weight, self.bias)


class LeakyReLU(nn.LeakyReLU):
    def forward(self, x):
        return TF.leaky_relu(x, self.negative_slope)


class ELU(nn.ELU):
    def forward(self, x):
        return TF.elu(x, self.alpha)


class SELU(nn.SELU):
    def forward(self, x):
        return TF.selu(x)


class Tanh(nn.Tanh):
    def forward(self, x):
        return TF.tanh(x)


class Sigmoid(nn.Sigmoid):
    """Parameter-free place holder that keeps the reference's ``Sequential(Linear, Sigmoid)`` layouts (state_dict keys
    ``masks.0.*``, models/blocks/scene.py:103-106).  Its one user, ``SceneStructureBlock``, hands the Linear's raw output to
    ``TF.scene_patches``, which evaluates the sigmoid inside the kernel; there is no stand-alone sigmoid kernel."""

    def forward(self, x):
        raise NotImplementedError('tartangan_amd.Sigmoid is fused into functional.scene_patches; it has no kernel of its own')


class AvgPool2d(nn.AvgPool2d):
    def __init__(self, kernel_size, **kw):
        super().__init__(kernel_size, **kw)
        if kernel_size not in (2, (2, 2)):
            raise ValueError('tartangan_amd.AvgPool2d supports kernel_size=2 only')

    def forward(self, x):
        return TF.avg_pool2(x)


class BatchNorm2d(nn.BatchNorm2d):
    """Train-mode batch statistics or eval-mode running statistics; ``forward_act``
    fuses the LeakyReLU that follows it in every reference block.  ``sync_group`` (a ``functional.SyncGroup``, set by
    ``parallel.DataParallel(sync_bn=True)``; never pickled) makes the training statistics those of the GLOBAL batch."""
    sync_group = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('sync_group', None)          # process-group handles do not travel with a checkpoint
        return state

    def _run(self, x, slope, replicate=1):
        if self.momentum is None or not self.affine or not self.track_running_stats:
            raise NotImplementedError('tartangan_amd.BatchNorm2d: default nn.BatchNorm2d options only')
        return TF.batch_norm_act(x, self.weight, self.bias, self.running_mean, self.running_var,
                                 self.training, self.momentum, self.eps, slope,
                                 self.num_batches_tracked if self.training else None, replicate, self.sync_group)

    def forward(self, x):
        return self._run(x, 1.0)

    def forward_act(self, x, slope, replicate=1):
        """BatchNorm + LeakyReLU(slope); ``replicate`` = 4 when ``x`` is the low-resolution source of a nearest x2
        upsampled tensor that the reference would have normalised (identical statistics, a quarter of the traffic)."""
        return self._run(x, slope, replicate)


class Conv1d(nn.Conv1d):
    """nn.Conv1d as the text trainer's blocks use it (conv_factory=nn.Conv1d): k=3/pad 1 or k=1/pad 0, stride 1, over (B, C, L)."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, bias=True, **kw):
        super().__init__(in_channels, out_channels, kernel_size, padding=padding, bias=bias, **kw)
        ks = self.kernel_size
        ok = (ks in ((1,), (3,)) and self.padding == (ks[0] // 2,) and self.stride == (1,) and self.dilation == (1,) and self.groups == 1)
        if not ok:
            raise ValueError(f'tartangan_amd.Conv1d supports k=3/pad1 and k=1/pad0 stride-1 only, got {self}')

    def forward(self, x, residual=None):
        return TF.conv1d(x, self.weight, self.bias, residual)


class AvgPool1d(nn.AvgPool1d):
    def __init__(self, kernel_size, **kw):
        super().__init__(kernel_size, **kw)
        if kernel_size not in (2, (2,)):
            raise ValueError('tartangan_amd.AvgPool1d supports kernel_size=2 only')

    def forward(self, x, residual=None):
        return TF.avg_pool2_1d(x, residual)


class BatchNorm1d(nn.BatchNorm1d):
    """nn.BatchNorm1d over (B, C, L) through the BatchNorm entry points with HW = L; ``forward_act`` as ``BatchNorm2d``."""

    def _run(self, x, slope):
        if self.momentum is None or not self.affine or not self.track_running_stats:
            raise NotImplementedError('tartangan_amd.BatchNorm1d: default nn.BatchNorm1d options only')
        if x.dim() != 3:
            raise NotImplementedError('tartangan_amd.BatchNorm1d takes (B, C, L)')
        return TF.batch_norm_act(x, self.weight, self.bias, self.running_mean, self.running_var, self.training, self.momentum,
                                 self.eps, slope, self.num_batches_tracked if self.training else None)

    def forward(self, x):
        return self._run(x, 1.0)

    def forward_act(self, x, slope):
        return self._run(x, slope)


def run_layers(seq, x, residual=None, residual_up=False):
    """Apply an ``nn.Sequential`` the way ``Sequential.forward`` would, fusing each
    (BatchNorm2d, LeakyReLU) pair into one kernel pass.  ``residual`` (the block's shortcut) is added to the
    result; when the last layer is a Conv2d or an AvgPool2d the add rides in that kernel's epilogue.
    ``residual_up``: the shortcut is given at half the resolution of the result (generator blocks); a final 3x3 Conv2d adds it
    upsampled on the fly, anything else gets it upsampled first."""
    mods = list(seq)
    if residual_up and not (mods and fusable_conv(mods[-1]) and mods[-1].kernel_size == (3, 3)):
        residual, residual_up = TF.upsample_nearest2x(residual), False
    i = 0
    while i < len(mods):
        m = mods[i]
        last = i == len(mods) - 1
        if last and residual is not None and type(m) in (Conv1d, AvgPool1d):
            # (B, C, L), the text trainer: the shortcut add rides in the 1-D kernel's epilogue
            x, residual = m(x, residual), None
            i += 1
            continue
        if (isinstance(m, (BatchNorm2d, BatchNorm1d)) and i + 1 < len(mods) and isinstance(mods[i + 1], LeakyReLU)):
            x = m.forward_act(x, mods[i + 1].negative_slope)
            i += 2
            continue
        if (i == len(mods) - 2 and fusable_conv(m) and type(mods[i + 1]) is AvgPool2d and m.kernel_size == (3, 3)
                and x.dim() == 4 and TF.pool_conv3x3_supported(x, m.weight if type(m) is Conv2d else m.weight_orig)):
            # conv3x3 -> AvgPool2d(2) [+ shortcut]: one 4x4-tap stride-2 convolution (2.25x fewer FLOPs, no full-resolution
            # conv output, no pool pass)
            x, residual = TF.pool_conv3x3(x, conv_weight(m), m.bias, residual), None
            i += 2
            continue
        if last and residual is not None and fusable_conv(m):
            x, residual = TF.conv2d(x, conv_weight(m), m.bias, residual, residual_up), None
        elif last and residual is not None and type(m) is AvgPool2d:
            x, residual = TF.avg_pool2(x, residual), None
        else:
            x = m(x)
        i += 1
    if residual is not None:
        x = TF.add(residual, x)
    return x


class Interpolate(nn.Module):
    """models/layers.py:6-14 for the two resamplings the hot path uses."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.args = args
        self.kwargs = kwargs

    def forward(self, x):
        return interpolate(x, *self.args, **self.kwargs)


def interpolate(x, size=None, scale_factor=None, mode='nearest', align_corners=None):
    """F.interpolate for (scale 2, nearest), (scale .5, bilinear, align_corners=True) and (scale 2, bilinear, align_corners=True)."""
    if not TF._is_pair(x) and x.dim() == 3:
        # (B, C, L), the text trainer: nearest x2, and the discriminator block's linear x0.5 without align_corners, which on an
        # even length is the average of each pair of tokens
        if size is None and scale_factor == 2 and mode == 'nearest':
            return TF.upsample_nearest2x_1d(x)
        if size is None and scale_factor == 0.5 and mode == 'linear' and not align_corners:
            if x.shape[2] % 2:
                raise NotImplementedError('interpolate(scale_factor=0.5, mode="linear") needs an even length')
            return TF.avg_pool2_1d(x)
        raise NotImplementedError(f'interpolate(scale_factor={scale_factor}, mode={mode}, align_corners={align_corners}) on (B, C, L) '
                                  f'is outside the hot path')
    if size is None and scale_factor == 2 and mode == 'nearest':
        return TF.upsample_nearest2x(x)
    if size is None and scale_factor == 2 and mode == 'bilinear' and align_corners:
        return TF.bilinear_up2x(x)
    if size is None and scale_factor == 0.5 and mode == 'bilinear' and align_corners:
        return TF.bilinear_half(x)
    raise NotImplementedError(f'interpolate(scale_factor={scale_factor}, mode={mode}, '
                              f'align_corners={align_corners}) is outside the hot path')


class PixelNorm(nn.Module):
    """models/layers.py:17-22 -- not on the cnn/iqn hot path; kept for API parity."""

    def __init__(self, eps=1e-8):
        super().__init__()
        self.eps = eps

    def forward(self, x):
        raise NotImplementedError('PixelNorm is not used by trainers.cnn / trainers.iqn')


default_activation = functools.partial(LeakyReLU, 0.2)
