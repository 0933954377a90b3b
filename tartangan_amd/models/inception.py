"""Inception-v3 forward on the HIP engine: the network between ``inception_preprocess`` and the FID / Inception-score math.

``Inception3`` is a drop-in for ``torchvision.models.inception_v3(transform_input=False)`` in eval mode: the same module
tree, ``state_dict`` keys and shapes (so the published ``inception_v3_google-*.pth`` loads, with or without its
``AuxLogits.*`` entries, which are never executed), but no layer has a ``forward`` of its own.  The whole network is one
stream of ``tg_inception_*`` launches driven by a plan:

* packing (first use, and again whenever a parameter or buffer was replaced or written: ``load_state_dict``, ``.to()``,
  ...): every BatchNorm is folded into its convolution in float64 on the host (``w * gamma / sqrt(var + eps)`` into the filter,
  ``beta - mean * gamma / sqrt(var + eps)`` into the bias), rounded to fp32 once and laid out K-major for the kernel
  (include/tartangan_amd.h).  1x1 branches of a Mixed block that read the same input and feed further convolutions are
  stacked into one launch;
* the plan (per input size): per layer the shape, the channel-slice offsets and the buffer ids.  Branches write straight into
  their slice of the block's concatenated output, so there is no ``torch.cat``;
* activation buffers: two that ping-pong between blocks and three for the inside of a block, sized for the batch and cached.
  After the first call at a batch size ``forward`` allocates nothing and never synchronises with the host, so it can be
  captured by ``torch.cuda.graph`` (one stream, no parallel branches).  The returned tensors are those cached buffers:
  they are overwritten by the next call at the same batch size (``WrapInception`` hands out copies).

Forward only; there is no CPU path (tests install the emulator backend)."""
import torch
from torch import nn

from .. import backend as _be

BN_EPS = 0.001


def K():
    return _be.get()


class BasicConv2d(nn.Module):
    """conv (no bias) -> BatchNorm2d(eps=0.001) -> ReLU; a parameter holder, executed by ``Inception3``'s plan."""

    def __init__(self, in_channels, out_channels, **kw):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, bias=False, **kw)
        self.bn = nn.BatchNorm2d(out_channels, eps=BN_EPS)


class InceptionA(nn.Module):
    def __init__(self, in_channels, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(in_channels, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(in_channels, pool_features, kernel_size=1)

    def plan(self, p, x, out):
        y = p.new(out, 64 + 64 + 96 + self.branch_pool.conv.out_channels, x.H, x.W)
        p.conv(x, [self.branch1x1], y.slice(0, 64))
        t = p.conv(x, [self.branch5x5_1, self.branch3x3dbl_1], p.new('t0', 48 + 64, x.H, x.W))
        p.conv(t.slice(0, 48), [self.branch5x5_2], y.slice(64, 64))
        u = p.conv(t.slice(48, 64), [self.branch3x3dbl_2], p.new('t1', 96, x.H, x.W))
        p.conv(u, [self.branch3x3dbl_3], y.slice(128, 96))
        a = p.avgpool(x, p.new('t2', x.C, x.H, x.W))
        p.conv(a, [self.branch_pool], y.slice(224, y.C - 224))
        return y


class InceptionB(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3 = BasicConv2d(in_channels, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def plan(self, p, x, out):
        oh, ow = (x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1
        y = p.new(out, 384 + 96 + x.C, oh, ow)
        p.conv(x, [self.branch3x3], y.slice(0, 384))
        t = p.conv(x, [self.branch3x3dbl_1], p.new('t0', 64, x.H, x.W))
        u = p.conv(t, [self.branch3x3dbl_2], p.new('t1', 96, x.H, x.W))
        p.conv(u, [self.branch3x3dbl_3], y.slice(384, 96))
        p.maxpool(x, y.slice(480, x.C))
        return y


class InceptionC(nn.Module):
    def __init__(self, in_channels, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)

    def plan(self, p, x, out):
        c7 = self.branch7x7_1.conv.out_channels
        y = p.new(out, 4 * 192, x.H, x.W)
        p.conv(x, [self.branch1x1], y.slice(0, 192))
        t = p.conv(x, [self.branch7x7_1, self.branch7x7dbl_1], p.new('t0', 2 * c7, x.H, x.W))
        u = p.conv(t.slice(0, c7), [self.branch7x7_2], p.new('t1', c7, x.H, x.W))
        p.conv(u, [self.branch7x7_3], y.slice(192, 192))
        u = p.conv(t.slice(c7, c7), [self.branch7x7dbl_2], p.new('t1', c7, x.H, x.W))
        v = p.conv(u, [self.branch7x7dbl_3], p.new('t2', c7, x.H, x.W))
        u = p.conv(v, [self.branch7x7dbl_4], p.new('t1', c7, x.H, x.W))
        p.conv(u, [self.branch7x7dbl_5], y.slice(384, 192))
        a = p.avgpool(x, p.new('t0', x.C, x.H, x.W))
        p.conv(a, [self.branch_pool], y.slice(576, 192))
        return y


class InceptionD(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def plan(self, p, x, out):
        oh, ow = (x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1
        y = p.new(out, 320 + 192 + x.C, oh, ow)
        t = p.conv(x, [self.branch3x3_1, self.branch7x7x3_1], p.new('t0', 384, x.H, x.W))
        p.conv(t.slice(0, 192), [self.branch3x3_2], y.slice(0, 320))
        u = p.conv(t.slice(192, 192), [self.branch7x7x3_2], p.new('t1', 192, x.H, x.W))
        v = p.conv(u, [self.branch7x7x3_3], p.new('t2', 192, x.H, x.W))
        p.conv(v, [self.branch7x7x3_4], y.slice(320, 192))
        p.maxpool(x, y.slice(512, x.C))
        return y


class InceptionE(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(in_channels, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)

    def plan(self, p, x, out):
        y = p.new(out, 320 + 768 + 768 + 192, x.H, x.W)
        p.conv(x, [self.branch1x1], y.slice(0, 320))
        t = p.conv(x, [self.branch3x3_1, self.branch3x3dbl_1], p.new('t0', 384 + 448, x.H, x.W))
        p.conv(t.slice(0, 384), [self.branch3x3_2a], y.slice(320, 384))
        p.conv(t.slice(0, 384), [self.branch3x3_2b], y.slice(704, 384))
        u = p.conv(t.slice(384, 448), [self.branch3x3dbl_2], p.new('t1', 384, x.H, x.W))
        p.conv(u, [self.branch3x3dbl_3a], y.slice(1088, 384))
        p.conv(u, [self.branch3x3dbl_3b], y.slice(1472, 384))
        a = p.avgpool(x, p.new('t2', x.C, x.H, x.W))
        p.conv(a, [self.branch_pool], y.slice(1856, 192))
        return y


class InceptionAux(nn.Module):
    """The auxiliary classifier: present so that the published state dict loads and the parameter count is torchvision's;
    never executed (torchvision runs it in training mode only)."""

    def __init__(self, in_channels, num_classes):
        super().__init__()
        self.conv0 = BasicConv2d(in_channels, 128, kernel_size=1)
        self.conv1 = BasicConv2d(128, 768, kernel_size=5)
        self.fc = nn.Linear(768, num_classes)


class _View:
    """Channels [coff, coff + C) of the (B, ctot, H, W) tensor kept in buffer ``buf``."""
    __slots__ = ('buf', 'ctot', 'coff', 'C', 'H', 'W')

    def __init__(self, buf, ctot, coff, C, H, W):
        self.buf, self.ctot, self.coff, self.C, self.H, self.W = buf, ctot, coff, C, H, W

    def slice(self, off, C):
        assert 0 <= off and off + C <= self.C, (off, C, self.C)
        return _View(self.buf, self.ctot, self.coff + off, C, self.H, self.W)


class _Plan:
    """Launch list for one input size.  ``ops``: ('conv', group, src, dst, Cin, Cout, H, W, KH, KW, stride, ph, pw, x_ctot,
    x_coff, y_ctot, y_coff) / ('maxpool' | 'avgpool', src, dst, C, H, W, x_ctot, x_coff, y_ctot, y_coff); ``groups``: the
    BasicConv2d modules behind each conv launch (several = stacked along Cout); ``floats``: buffer id -> floats per image."""

    def __init__(self):
        self.ops, self.groups, self.floats, self.macs = [], [], {}, 0

    def new(self, buf, C, H, W):
        self.floats[buf] = max(self.floats.get(buf, 0), C * H * W)
        return _View(buf, C, 0, C, H, W)

    def conv(self, x, mods, y):
        c0 = mods[0].conv
        KH, KW = c0.kernel_size
        (sh, sw), (ph, pw) = c0.stride, c0.padding
        for m in mods:
            c = m.conv
            assert (c.in_channels, c.kernel_size, c.stride, c.padding) == (c0.in_channels, c0.kernel_size, c0.stride, c0.padding)
            assert c.dilation == (1, 1) and c.groups == 1 and c.bias is None
        cout = sum(m.conv.out_channels for m in mods)
        oh, ow = (x.H + 2 * ph - KH) // sh + 1, (x.W + 2 * pw - KW) // sw + 1
        assert sh == sw and x.C == c0.in_channels and y.C == cout and (y.H, y.W) == (oh, ow) and oh > 0 and ow > 0, \
            (x.C, c0.in_channels, y.C, cout, (y.H, y.W), (oh, ow))
        self.groups.append(list(mods))
        self.ops.append(('conv', len(self.groups) - 1, x.buf, y.buf, x.C, cout, x.H, x.W, KH, KW, sh, ph, pw,
                         x.ctot, x.coff, y.ctot, y.coff))
        self.macs += cout * x.C * KH * KW * oh * ow
        return y

    def maxpool(self, x, y):
        assert x.H >= 3 and x.W >= 3 and y.C == x.C and (y.H, y.W) == ((x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1)
        self.ops.append(('maxpool', x.buf, y.buf, x.C, x.H, x.W, x.ctot, x.coff, y.ctot, y.coff))
        return y

    def avgpool(self, x, y):
        assert y.C == x.C and (y.H, y.W) == (x.H, x.W)
        self.ops.append(('avgpool', x.buf, y.buf, x.C, x.H, x.W, x.ctot, x.coff, y.ctot, y.coff))
        return y


def pack_conv(mods):
    """BatchNorm folded into the stacked filters of ``mods`` in float64 -> (wp (Kp, CoutP) fp32, bias (Cout) fp32), CPU, in the
    layout tg_inception_conv_fwd reads (include/tartangan_amd.h)."""
    ws, bs = [], []
    for m in mods:
        w = m.conv.weight.detach().double().cpu()
        scale = m.bn.weight.detach().double().cpu() / torch.sqrt(m.bn.running_var.detach().double().cpu() + m.bn.eps)
        ws.append(w * scale.view(-1, 1, 1, 1))
        bs.append(m.bn.bias.detach().double().cpu() - m.bn.running_mean.detach().double().cpu() * scale)
    w = torch.cat(ws, 0)
    cout, k = w.shape[0], w[0].numel()
    kp, coutp = -(-k // 16) * 16, -(-cout // 128) * 128
    wp = torch.zeros(kp, coutp, dtype=torch.float64)
    wp[:k, :cout] = w.reshape(cout, k).t()
    return wp.float().contiguous(), torch.cat(bs).float().contiguous()


class Inception3(nn.Module):
    STEM = ('Conv2d_1a_3x3', 'Conv2d_2a_3x3', 'Conv2d_2b_3x3', 'pool', 'Conv2d_3b_1x1', 'Conv2d_4a_3x3', 'pool')
    MIXED = ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e', 'Mixed_7a',
             'Mixed_7b', 'Mixed_7c')

    def __init__(self, num_classes=1000, aux_logits=True):
        super().__init__()
        self.aux_logits = aux_logits
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, pool_features=32)
        self.Mixed_5c = InceptionA(256, pool_features=64)
        self.Mixed_5d = InceptionA(288, pool_features=64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, channels_7x7=128)
        self.Mixed_6c = InceptionC(768, channels_7x7=160)
        self.Mixed_6d = InceptionC(768, channels_7x7=160)
        self.Mixed_6e = InceptionC(768, channels_7x7=192)
        if aux_logits:
            self.AuxLogits = InceptionAux(768, num_classes)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)
        self.fc = nn.Linear(2048, num_classes)
        for p in self.parameters():
            p.requires_grad_(False)
        self._packed_sig, self._packed, self._plans, self._act_buffers = None, None, {}, {}
        super().train(False)

    # ------------------------------------------------------------------------------------------------ nn.Module surface
    def train(self, mode=True):
        """Eval only: the running statistics are folded into the filters."""
        return super().train(False)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Accepts torchvision's keys with or without the ``AuxLogits.*`` entries."""
        has_aux = any(k.startswith('AuxLogits.') for k in state_dict)
        if has_aux != self.aux_logits:
            state_dict = {k: v for k, v in state_dict.items() if not k.startswith('AuxLogits.')}
            if self.aux_logits:
                state_dict.update({k: v for k, v in self.state_dict().items() if k.startswith('AuxLogits.')})
        return super().load_state_dict(state_dict, strict=strict, **kw)

    # ------------------------------------------------------------------------------------------------ plan and packing
    def plan(self, H=299, W=299):
        """The launch plan for (., 3, H, W) inputs (cached)."""
        key = (H, W)
        if key not in self._plans:
            p = _Plan()
            x = _View('x', 3, 0, 3, H, W)
            bufs = ('a', 'b')
            n = 0
            for name in self.STEM:
                if name == 'pool':
                    if x.H < 3 or x.W < 3:
                        raise ValueError(f'Inception3: a {H} x {W} input is too small (75 x 75 is the minimum)')
                    x = p.maxpool(x, p.new(bufs[n % 2], x.C, (x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1))
                else:
                    c = getattr(self, name).conv
                    oh = (x.H + 2 * c.padding[0] - c.kernel_size[0]) // c.stride[0] + 1
                    ow = (x.W + 2 * c.padding[1] - c.kernel_size[1]) // c.stride[1] + 1
                    if oh <= 0 or ow <= 0:
                        raise ValueError(f'Inception3: a {H} x {W} input is too small (75 x 75 is the minimum)')
                    x = p.conv(x, [getattr(self, name)], p.new(bufs[n % 2], c.out_channels, oh, ow))
                n += 1
            for name in self.MIXED:
                if isinstance(getattr(self, name), (InceptionB, InceptionD)) and (x.H < 3 or x.W < 3):
                    raise ValueError(f'Inception3: a {H} x {W} input is too small (75 x 75 is the minimum)')
                x = getattr(self, name).plan(p, x, bufs[n % 2])
                n += 1
            p.out = x
            p.macs += self.fc.in_features * self.fc.out_features
            self._plans[key] = p
        return self._plans[key]

    def _signature(self):
        """What the packed filters were made from: identity, version counter and address of every executed tensor.  Checked on
        every forward (host only, no synchronisation), so it reads the leaf modules' own dicts instead of walking the tree."""
        leaves = self.__dict__.get('_leaves')
        if leaves is None:
            leaves = [m for n, m in self.named_modules() if not n.startswith('AuxLogits') and (m._parameters or m._buffers)]
            self.__dict__['_leaves'] = leaves
        return tuple((id(t), t._version, t.data_ptr()) for m in leaves for d in (m._parameters, m._buffers)
                     for t in d.values() if t is not None)

    def _pack(self, plan):
        """Folded, packed filters of every launch of ``plan`` on the parameters' device; redone when a tensor changed."""
        sig = self._signature()
        if self._packed_sig != sig:
            self._packed, self._packed_sig = {}, sig
        packed = self._packed.get(id(plan))
        if packed is None:
            dev = self.fc.weight.device
            packed = [tuple(t.to(dev) for t in pack_conv(mods)) for mods in plan.groups]
            for (wp, _), mods in zip(packed, plan.groups):
                c = mods[0].conv
                need = K().inception_conv_weight_floats(c.in_channels, sum(m.conv.out_channels for m in mods), *c.kernel_size)
                assert wp.numel() == need, (wp.shape, need)
            self._packed[id(plan)] = packed
        return packed

    def _get_buffers(self, plan, B, device):
        key = (id(plan), B, str(device))
        got = self._act_buffers.get(key)
        if got is None:
            got = {name: torch.empty(B * n, dtype=torch.float32, device=device) for name, n in plan.floats.items()}
            got['pool'] = torch.empty(B, self.fc.in_features, dtype=torch.float32, device=device)
            got['logits'] = torch.empty(B, self.fc.out_features, dtype=torch.float32, device=device)
            self._act_buffers[key] = got
        return got

    # ------------------------------------------------------------------------------------------------ forward
    def _run(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f'Inception3 takes a normalised (B, 3, H, W) tensor, got {tuple(x.shape)}')
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError('Inception3 is forward-only (no backward through the native Inception network): call it under '
                               'torch.no_grad() or detach the input')
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        if x.device != self.fc.weight.device:
            raise RuntimeError(f'Inception3: input on {x.device}, parameters on {self.fc.weight.device}')
        B, _, H, W = x.shape
        plan = self.plan(H, W)
        packed = self._pack(plan)
        bufs = dict(self._get_buffers(plan, B, x.device))
        bufs['x'] = x
        k = K()
        for op in plan.ops:
            if op[0] == 'conv':
                _, g, src, dst, cin, cout, h, w, kh, kw, stride, ph, pw, xct, xco, yct, yco = op
                if not k.inception_conv_supported(B, cin, cout, h, w, kh, kw, stride, ph, pw, xct, yct):
                    raise _be.KernelError(f'tg_inception_conv_fwd does not cover {op[4:]} at batch {B}')
                wp, bias = packed[g]
                k.inception_conv_fwd(bufs[src], wp, bias, bufs[dst], B, cin, cout, h, w, kh, kw, stride, ph, pw, 1, xct, xco, yct, yco)
            else:
                kind, src, dst, c, h, w, xct, xco, yct, yco = op
                (k.inception_maxpool3s2 if kind == 'maxpool' else k.inception_avgpool3)(bufs[src], bufs[dst], B, c, h, w, xct, xco, yct, yco)
        o = plan.out
        return bufs, bufs[o.buf][:B * o.C * o.H * o.W].view(B, o.C, o.H, o.W)

    def features(self, x):
        """The (B, 2048, 8, 8) map in front of the global pool (a cached buffer: valid until the next call)."""
        return self._run(x)[1]

    def forward(self, x):
        """Normalised (B, 3, 299, 299) -> (pool (B, 2048), logits (B, num_classes)); cached buffers, valid until the next call."""
        bufs, feat = self._run(x)
        B, C, H, W = feat.shape
        pool, logits = bufs['pool'], bufs['logits']
        k = K()
        k.row_sum(feat, pool, 1.0 / (H * W), B * C, H * W)
        n = self.fc.out_features
        k.gemm(pool, self.fc.weight, logits, self.fc.bias, B, n, C, C, C, n, 0, 1, 1, 0, 0, 0, 0.0)      # dropout: identity in eval
        return pool, logits

    def macs(self, H=299, W=299):
        """Multiply-accumulates of one image through the plan (convolutions and fc)."""
        return self.plan(H, W).macs
