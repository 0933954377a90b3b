"""Helpers of the Inception-v3 tests (not collected).

* ``RefInception3``: the eval-mode forward of Inception-v3 restated with stock torch modules (``nn.Conv2d`` /
  ``nn.BatchNorm2d`` / ``F.relu`` / ``F.max_pool2d`` / ``F.avg_pool2d`` / ``torch.cat`` / ``nn.Linear``) under torchvision's
  module names, written from the published architecture (Szegedy et al. 2015, "Rethinking the Inception Architecture", as
  torchvision lays it out).  Its ``state_dict`` loads into ``tartangan_amd.models.inception.Inception3`` and back; it runs in
  float64 (the truth) and in float32 (what plain fp32 arithmetic achieves).
* ``procedural_state``: weights from a seed under which activations neither die nor blow up through the network's depth; and
  ``check_reference_health``, the assertion of that on the float64 run (a condition on the reference alone).
* ``InceptionEmulator``: ``tests/emulator.Emulator`` plus the ``tg_inception_*`` entry points in torch CPU ops, so the host
  logic (BatchNorm folding, slice offsets, plan order, buffers) runs without a GPU."""
import torch
import torch.nn.functional as F
from torch import nn

from emulator import Emulator


# ------------------------------------------------------------------------------------------------------ the restatement
class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, kernel_size=1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b5 = self.branch5x5_2(self.branch5x5_1(x))
        b3 = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b5, b3, bp], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        b3 = self.branch3x3(x)
        bd = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_1(x)
        for name in ('branch7x7dbl_2', 'branch7x7dbl_3', 'branch7x7dbl_4', 'branch7x7dbl_5'):
            bd = getattr(self, name)(bd)
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b7, bd, bp], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        b3 = self.branch3x3_2(self.branch3x3_1(x))
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b3 = self.branch3x3_1(x)
        b3 = torch.cat([self.branch3x3_2a(b3), self.branch3x3_2b(b3)], 1)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bd = torch.cat([self.branch3x3dbl_3a(bd), self.branch3x3dbl_3b(bd)], 1)
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b3, bd, bp], 1)


class InceptionAux(nn.Module):
    def __init__(self, cin, num_classes):
        super().__init__()
        self.conv0 = BasicConv2d(cin, 128, kernel_size=1)
        self.conv1 = BasicConv2d(128, 768, kernel_size=5)
        self.fc = nn.Linear(768, num_classes)


class RefInception3(nn.Module):
    LAYERS = ('Conv2d_1a_3x3', 'Conv2d_2a_3x3', 'Conv2d_2b_3x3', 'pool', 'Conv2d_3b_1x1', 'Conv2d_4a_3x3', 'pool',
              'Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e',
              'Mixed_7a', 'Mixed_7b', 'Mixed_7c')

    def __init__(self, num_classes=1000, aux_logits=True):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        if aux_logits:
            self.AuxLogits = InceptionAux(768, num_classes)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)
        self.fc = nn.Linear(2048, num_classes)
        self.eval()

    def blocks(self, x):
        """Every stage's output, in order (the last one is the feature map in front of the global pool)."""
        outs = []
        for name in self.LAYERS:
            x = F.max_pool2d(x, kernel_size=3, stride=2) if name == 'pool' else getattr(self, name)(x)
            outs.append((name, x))
        return outs

    def features(self, x):
        return self.blocks(x)[-1][1]

    def forward(self, x):
        f = self.features(x)
        pool = torch.mean(f.view(f.size(0), f.size(1), -1), 2)
        return pool, self.fc(pool)


# --------------------------------------------------------------------------------------------------- procedural weights
def procedural_state(seed=0, aux=True, num_classes=1000):
    """A float32 state dict with torchvision's keys.  Convolutions: uniform with the He variance 2 / fan_in (a ReLU of a
    zero-mean unit-variance input keeps half the second moment); BatchNorm: gamma, running_var in [0.5, 1.5], beta and
    running_mean in [-0.1, 0.1], so the folded scale is of order one; fc: uniform with variance 0.05^2 / fan_in, so that the
    logits (a zero-mean mix of pooled features whose RMS may reach 20) stay of order one: a softmax that underflows to an
    exact zero makes the Inception score's p log p a NaN, in the reference's formula as much as here."""
    gen = torch.Generator().manual_seed(seed)
    ref = RefInception3(num_classes, aux_logits=aux)
    state = {}
    for key, t in ref.state_dict().items():
        if key.endswith('num_batches_tracked'):
            v = torch.zeros_like(t)
        elif key.endswith('conv.weight'):
            fan_in = t[0].numel()
            v = (torch.rand(t.shape, generator=gen) * 2 - 1) * (6.0 / fan_in) ** 0.5
        elif key.endswith('bn.weight') or key.endswith('running_var'):
            v = 0.5 + torch.rand(t.shape, generator=gen)
        elif key.endswith('bn.bias') or key.endswith('running_mean'):
            v = (torch.rand(t.shape, generator=gen) * 2 - 1) * 0.1
        elif key.endswith('fc.weight'):
            v = (torch.rand(t.shape, generator=gen) * 2 - 1) * 0.05 * (3.0 / t.shape[1]) ** 0.5
        else:
            assert key.endswith('fc.bias'), key
            v = (torch.rand(t.shape, generator=gen) * 2 - 1) * 0.1
        state[key] = v
    return state


def reference(state, dtype=torch.float64):
    ref = RefInception3(state['fc.weight'].shape[0], aux_logits=any(k.startswith('AuxLogits.') for k in state))
    ref.load_state_dict(state)
    return ref.to(dtype).eval()


def procedural_input(batch, size, seed=1):
    """Smooth, image-like normalised input: low-frequency waves plus noise, roughly zero mean and unit variance."""
    gen = torch.Generator().manual_seed(seed)
    ys = torch.linspace(0, 1, size).view(1, 1, size, 1)
    xs = torch.linspace(0, 1, size).view(1, 1, 1, size)
    f = torch.rand(batch, 3, 1, 1, generator=gen) * 6 + 1
    ph = torch.rand(batch, 3, 1, 1, generator=gen) * 6.28
    img = torch.sin(f * 6.28 * xs + ph) * torch.cos(f * 3.1 * ys - ph) + 0.5 * torch.randn(batch, 3, size, size, generator=gen)
    return img.float().contiguous()


def check_reference_health(ref64, x):
    """On the float64 reference: every stage's RMS within [0.05, 20] and under 90 % exact zeros; logits within +-30 (a soft
    softmax: no class probability underflows in fp32)."""
    with torch.no_grad():
        outs = ref64.blocks(x.double())
        logits = ref64.fc(outs[-1][1].mean((2, 3)))
    assert float(logits.abs().max()) < 30.0, f'logits reach {float(logits.abs().max()):.3g}'
    for name, t in outs:
        rms = float(t.pow(2).mean().sqrt())
        zeros = float((t == 0).double().mean())
        assert 0.05 <= rms <= 20.0, f'{name}: RMS {rms:.3g} outside [0.05, 20]'
        assert zeros < 0.9, f'{name}: {zeros:.1%} zeros'
    return outs


def results(net, x):
    """{'features', 'pool', 'logits'} of a network with ``features`` / ``forward``, as float64 CPU tensors."""
    with torch.no_grad():
        feat = net.features(x).detach().to('cpu', torch.float64).clone()
        pool, logits = net(x)
    return {'features': feat, 'pool': pool.detach().to('cpu', torch.float64).clone(),
            'logits': logits.detach().to('cpu', torch.float64).clone()}


# ------------------------------------------------------------------------------------------------------------- emulator
def _slice(t, B, ctot, coff, C, H, W):
    return t.reshape(-1)[:B * ctot * H * W].view(B, ctot, H, W)[:, coff:coff + C]


class InceptionEmulator(Emulator):
    def inception_conv_weight_floats(self, Cin, Cout, KH, KW):
        return (-(-(Cin * KH * KW) // 16) * 16) * (-(-Cout // 128) * 128)

    def inception_conv_supported(self, B, Cin, Cout, H, W, KH, KW, stride, ph, pw, x_ctot, y_ctot):
        return int(stride in (1, 2) and x_ctot >= Cin and y_ctot >= Cout)

    def inception_conv_fwd(self, x, wp, bias, y, B, Cin, Cout, H, W, KH, KW, stride, ph, pw, relu, x_ctot, x_coff, y_ctot, y_coff):
        K = Cin * KH * KW
        w = wp.view(-1, -(-Cout // 128) * 128)[:K, :Cout].t().reshape(Cout, Cin, KH, KW)
        r = F.conv2d(_slice(x, B, x_ctot, x_coff, Cin, H, W), w, bias, stride=stride, padding=(ph, pw))
        if relu:
            r = F.relu(r)
        _slice(y, B, y_ctot, y_coff, Cout, r.shape[2], r.shape[3]).copy_(r)
        return 0

    def inception_maxpool3s2(self, x, y, B, C, H, W, x_ctot, x_coff, y_ctot, y_coff):
        r = F.max_pool2d(_slice(x, B, x_ctot, x_coff, C, H, W), kernel_size=3, stride=2)
        _slice(y, B, y_ctot, y_coff, C, r.shape[2], r.shape[3]).copy_(r)
        return 0

    def inception_avgpool3(self, x, y, B, C, H, W, x_ctot, x_coff, y_ctot, y_coff):
        r = F.avg_pool2d(_slice(x, B, x_ctot, x_coff, C, H, W), kernel_size=3, stride=1, padding=1)
        _slice(y, B, y_ctot, y_coff, C, H, W).copy_(r)
        return 0
