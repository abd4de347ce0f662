"""DispHeadV2 from torch.nn modules (a test helper, written from the forward stated in include/stereotrack.h section 23):

    x = ELU(BN(conv3x3 in -> C)); x = ELU(BN(conv3x3 C -> C)); x = nearest x2(x)
    g = df * (1 - sigmoid(mlp(avgpool(df)) + mlp(maxpool(df))))      mlp = Linear(64, 16), ReLU, Linear(16, 64)
    x = cat(x, g); x = ELU(BN(conv3x3 C+64 -> 256)); x = ELU(BN(conv3x3 256 -> 256)); x = nearest x2(x)
    x = ELU(BN(conv3x3 256 -> 128)); y = ReLU(conv1x1 128 -> 1 + bias)
    rescale: bilinear, align_corners=False, to img_shape

The module tree yields the reference's state_dict keys (dconv1_1.conv.weight, dconv1_1.bn.running_var,
cbam.ChannelGate.mlp.1.weight, reg.conv.bias, ...).  Evaluated on the CPU in fp32 or fp64 (`.double()`).
"""
import functools
import zlib

import torch
import torch.nn as nn
import torch.nn.functional as F

TAPS = ('dconv1_2', 'gate_scale', 'cat', 'dconv2_2', 'dconv3_1_raw', 'pred')


class ConvBN(nn.Module):
    """conv3x3 (no bias) + BatchNorm2d(eps=1e-3) in eval mode; forward returns the RAW (pre-ELU) value."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=1e-3)

    def forward(self, x):
        return self.bn(self.conv(x))


class Reg(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(128, 1, 1, bias=True)

    def forward(self, x):
        return F.relu(self.conv(x))


class ChannelGate(nn.Module):
    def __init__(self):
        super().__init__()
        self.mlp = nn.Sequential(nn.Flatten(), nn.Linear(64, 16), nn.ReLU(), nn.Linear(16, 64))

    def scale(self, x):
        return torch.sigmoid(self.mlp(x.mean(dim=(2, 3))) + self.mlp(x.amax(dim=(2, 3))))

    def forward(self, x):
        return x * (1 - self.scale(x)[:, :, None, None])


class CBAM(nn.Module):
    def __init__(self):
        super().__init__()
        self.ChannelGate = ChannelGate()

    def forward(self, x):
        return self.ChannelGate(x)


class RefDispHead(nn.Module):
    def __init__(self, in_channels, channels):
        super().__init__()
        self.dconv1_1 = ConvBN(in_channels, channels)
        self.dconv1_2 = ConvBN(channels, channels)
        self.dconv2_1 = ConvBN(channels + 64, 256)
        self.dconv2_2 = ConvBN(256, 256)
        self.dconv3_1 = ConvBN(256, 128)
        self.reg = Reg()
        self.cbam = CBAM()
        self.eval()

    def forward(self, p3, df):
        """p3 (N,in,h,w), df (N,64,2h,2w) -> dict of the taps, NCHW (gate_scale (N,64)); 'pre_elu' = every raw
        conv + BN value in one vector."""
        t = {}
        a = self.dconv1_1(p3)
        t['dconv1_2'] = b = self.dconv1_2(F.elu(a))
        x = F.interpolate(F.elu(b), scale_factor=2, mode='nearest')
        t['gate_scale'] = self.cbam.ChannelGate.scale(df)
        t['cat'] = cat = torch.cat((x, self.cbam(df)), dim=1)
        d = self.dconv2_1(cat)
        t['dconv2_2'] = e = self.dconv2_2(F.elu(d))
        x = F.interpolate(F.elu(e), scale_factor=2, mode='nearest')
        t['dconv3_1_raw'] = g = self.dconv3_1(x)
        t['pre_reg'] = self.reg.conv(F.elu(g))
        t['pred'] = F.relu(t['pre_reg'])
        t['pre_elu'] = torch.cat([v.reshape(-1) for v in (a, b, d, e, g)])
        return t


def resize(pred, size):
    return F.interpolate(pred, size=tuple(size), mode='bilinear', align_corners=False)


def random_state_dict(in_channels, channels, seed):
    """Seeded weights with non-trivial BN statistics; the reg bias is 0 (make_case centres it)."""
    head = RefDispHead(in_channels, channels)
    g = torch.Generator()
    sd = {}
    for name, v in head.state_dict().items():
        g.manual_seed((zlib.crc32(name.encode()) + 7919 * int(seed)) & 0x7FFFFFFF)
        if name.endswith('num_batches_tracked'):
            continue
        if name.endswith('conv.weight'):
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            sd[name] = torch.randn(v.shape, generator=g) * (1.6 / fan_in ** 0.5)
        elif name.endswith(('bn.weight', 'running_var')):
            sd[name] = torch.rand(v.shape, generator=g) * 0.9 + 0.6
        elif name.endswith(('bn.bias', 'running_mean')):
            sd[name] = torch.randn(v.shape, generator=g) * 0.3
        elif 'mlp' in name and name.endswith('weight'):
            sd[name] = torch.randn(v.shape, generator=g) * (0.3 / v.shape[1] ** 0.5)
        elif 'mlp' in name:
            sd[name] = torch.randn(v.shape, generator=g) * 0.2
        else:                       # reg.conv.bias
            sd[name] = torch.zeros(v.shape)
    return sd


# (N, channels, p3 h, p3 w, in_channels, seed): the cases of the GPU test of the head alone
CASES = ((1, 32, 4, 4, 16, 11), (2, 64, 8, 12, 128, 12), (3, 96, 5, 7, 24, 13))


@functools.lru_cache(maxsize=None)
def make_case(N, C, h, w, in_channels, seed):
    """-> dict(sd, p3, df (NCHW fp32), ref64, ref32 (taps on the CPU in fp64 / fp32)).  The reg bias is set to minus the
    median of the fp64 pre-ReLU values, so about half of the prediction is an exact zero and half positive.  Computed
    once per case and shared: treat as read-only."""
    g = torch.Generator().manual_seed(1000 + seed)
    p3 = torch.randn(N, in_channels, h, w, generator=g)
    df = torch.randn(N, 64, 2 * h, 2 * w, generator=g) * 1.5 + 0.2
    sd = random_state_dict(in_channels, C, seed)
    head = RefDispHead(in_channels, C)
    head.load_state_dict(sd, strict=False)
    with torch.no_grad():
        pre = head.double()(p3.double(), df.double())['pre_reg']
        sd['reg.conv.bias'] = -pre.median().float().reshape(1)
        head.load_state_dict({k: v.double() for k, v in sd.items()}, strict=False)
        ref64 = head(p3.double(), df.double())
        head32 = RefDispHead(in_channels, C)
        head32.load_state_dict(sd, strict=False)
        ref32 = head32(p3, df)
    return dict(sd=sd, p3=p3, df=df, ref64=ref64, ref32=ref32)
