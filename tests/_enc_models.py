"""Small seeded encoders for tests/test_gpu_encoder_convs.py and tests/test_strided_ref_cpu.py, in the shape of the reference's
BasicEncoder and MultiBasicEncoder (models/raft_stereo/extractor.py:122-300) as vppstereo_amd/extractor.py documents it, with
channel counts the convolution kernel takes: 16 / 32 / 48, so that every convolution but the stem is a plain one.

TEST INFRASTRUCTURE ONLY.  torch is imported where it is used.

  stem    conv1 3 -> 16, 7x7, stride 1 (Cin = 3: never on the kernel), norm1
  layer1  16 -> 16 stride 1;  layer2  16 -> 32 stride 2;  layer3  32 -> 48 stride 2     (two ResidualBlocks each)
  basic   conv2 48 -> 32, 1x1; InstanceNorm2d
  multi   layer4, layer5 48 -> 48 stride 2; outputs08 / outputs16: two heads of (ResidualBlock 48 -> 48, Conv2d 48 -> 16 3x3) as in
          tests/_raft_loop.py; outputs32: two Conv2d 48 -> 16 3x3; BatchNorm2d in eval mode with seeded statistics

A [2,3,36,52] input gives maps of 36x52, 18x26, 9x13, 5x7 and 3x4: even and odd sizes at stride 2, more than one tile at the top.
"""
from _raft_loop import HIDDEN, _res_block

FEATURES = 32
INPUT = (2, 3, 36, 52)


def _trunk(nn, enc, norm):
    enc.conv1, enc.norm1 = nn.Conv2d(3, 16, 7, stride=1, padding=3), norm(16)
    enc.layer1 = nn.Sequential(_res_block(nn, 16, 16, norm, 1), _res_block(nn, 16, 16, norm, 1))
    enc.layer2 = nn.Sequential(_res_block(nn, 16, 32, norm, 2), _res_block(nn, 32, 32, norm, 1))
    enc.layer3 = nn.Sequential(_res_block(nn, 32, 48, norm, 2), _res_block(nn, 48, 48, norm, 1))


def _finish(torch, model, seed):
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 0.5 + 0.2)
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.2)
    for p in model.parameters():
        p.requires_grad_(False)
    return model.eval()


def basic(seed=6701):
    """-> an nn.Module in eval mode, float32, on the CPU, in the shape of BasicEncoder(norm_fn='instance')."""
    import torch
    nn = torch.nn
    torch.manual_seed(seed)
    enc = nn.Module()
    _trunk(nn, enc, lambda c: nn.InstanceNorm2d(c))
    enc.conv2 = nn.Conv2d(48, FEATURES, 1)
    return _finish(torch, enc, seed)


def multi(seed=6702):
    """-> the same in the shape of MultiBasicEncoder(norm_fn='batch'), its BatchNorms frozen."""
    import torch
    nn = torch.nn
    torch.manual_seed(seed)
    bnorm = lambda c: nn.BatchNorm2d(c)                                                 # noqa: E731
    enc = nn.Module()
    _trunk(nn, enc, bnorm)
    enc.layer4 = nn.Sequential(_res_block(nn, 48, 48, bnorm, 2), _res_block(nn, 48, 48, bnorm, 1))
    enc.layer5 = nn.Sequential(_res_block(nn, 48, 48, bnorm, 2), _res_block(nn, 48, 48, bnorm, 1))
    head = lambda: nn.Sequential(_res_block(nn, 48, 48, bnorm, 1), nn.Conv2d(48, HIDDEN, 3, padding=1))     # noqa: E731
    enc.outputs08 = nn.ModuleList([head(), head()])
    enc.outputs16 = nn.ModuleList([head(), head()])
    enc.outputs32 = nn.ModuleList([nn.Conv2d(48, HIDDEN, 3, padding=1), nn.Conv2d(48, HIDDEN, 3, padding=1)])
    return _finish(torch, enc, seed)


def convs_of(enc):
    """Every nn.Conv2d of the encoder but the stem: the convolutions FusedEncoder(convs=True) runs on the kernel."""
    import torch
    return [m for m in enc.modules() if isinstance(m, torch.nn.Conv2d) and m is not enc.conv1]


def image(device, seed=6703, shape=INPUT):
    import torch
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(device)


def plain(enc, x):
    """The encoder in plain torch operations -> a flat list of its outputs (basic: [features]; multi: outputs08 + 16 + 32)."""
    import _raft_loop as L
    if hasattr(enc, "outputs08"):
        return [t for group in L._plain_cnet(enc, x) for t in group]
    return [enc.conv2(L._plain_trunk(enc, x))]


def flat(out):
    """What FusedEncoder.forward returned as the same flat list."""
    if hasattr(out, "shape"):
        return [out]
    return [t for group in out for t in group]
