"""Golden vectors for PSMNet's feature_extraction on the library's kernels, produced by running the REFERENCE's own modules
(models/psmnet/submodule.py) on the CPU (the tests read the recording, not the reference):

  * a.*: BasicBlock(16, 16, 1, None, 1, 2) -- the reference's own block at dilation 2, as layer4 has it;
  * b.*: BasicBlock(16, 32, 2, downsample, 1, 1) with a convbn(16, 32, 1, 2, 0, 1) downsample, as layer2[0] has it;
    both on a 9x13 map with B = 2, in eval mode, with seeded BatchNorm running statistics and affine parameters and convolution
    weights scaled so that sums are of order 1.  Per block the input, the state dict (key for key) and the output.
  * tail.*: the reference's own feature_extraction.forward (:201-253) with firstconv, layer1, layer3 and lastconv replaced by
    identities and layer2, layer4 by 1x1 convolutions to 64 and 128 channels whose weights are the integer formulas below, so
    that the reference's pool, branch, interpolate and cat lines run on a 64 x 72 map, the smallest AvgPool2d(64) takes.  The input
    is an integer formula as well (tests/test_gpu_psm_features.py repeats all three, exact in float32).  Stored: the four branches'
    parameters and, of the [1,320,64,72] result, rows TAIL_ROWS of the 128 branch channels and of channels TAIL_HEADS.

Arrays only.  Run:  python tests/golden/make_psm_golden.py REFERENCE_ROOT     (writes tests/golden/psm_cases.npz)
"""
import os
import sys
import warnings

import numpy as np
import torch

REF = sys.argv[1]                             # root of a checkout of the reference
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import models.psmnet.submodule as SM  # noqa: E402

TAIL_ROWS = (0, 7, 8, 31, 32, 47, 48, 63)
TAIL_HEADS = (0, 63, 64, 191)


def tail_input():
    """[1,4,64,72]: multiples of 1/8 between -15/8 and 15/8."""
    c, y, x = np.meshgrid(np.arange(4), np.arange(64), np.arange(72), indexing="ij")
    return (((7 * y + 13 * x + 29 * c) % 31 - 15) / 8.0).astype(np.float32)[None]


def tail_weights():
    """layer2's stand-in [64,4,1,1] and layer4's [128,64,1,1]."""
    m, c = np.meshgrid(np.arange(64), np.arange(4), indexing="ij")
    w2 = (((5 * m + 3 * c) % 17 - 8) / 16.0).astype(np.float32)[:, :, None, None]
    m, c = np.meshgrid(np.arange(128), np.arange(64), indexing="ij")
    w4 = (((7 * m + 11 * c) % 19 - 9) / 64.0).astype(np.float32)[:, :, None, None]
    return w2, w4


def seed_module(mod, gen):
    """Seeded BatchNorm statistics and affine parameters; convolution weights of about 1.5 / sqrt(K)."""
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.Conv2d):
                K = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (1.5 / K ** 0.5))
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.5)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.num_features, generator=gen))
                m.bias.copy_(0.3 * torch.randn(m.num_features, generator=gen))
    return mod.eval()


if __name__ == "__main__":
    gen = torch.Generator().manual_seed(7401)
    rng = np.random.default_rng(7402)
    out = {}
    blocks = {"a": SM.BasicBlock(16, 16, 1, None, 1, 2), "b": SM.BasicBlock(16, 32, 2, SM.convbn(16, 32, 1, 2, 0, 1), 1, 1)}
    for name, blk in blocks.items():
        seed_module(blk, gen)
        x = torch.from_numpy(np.tanh(rng.standard_normal((2, 16, 9, 13))).astype(np.float32))
        with torch.no_grad():
            y = blk(x.clone())
        out.update({f"{name}.{k}": v.detach().numpy().copy() for k, v in blk.state_dict().items()})
        out[f"{name}.x"], out[f"{name}.out"] = x.numpy().copy(), y.numpy().copy()

    fe = SM.feature_extraction()
    seed_module(fe, gen)
    w2, w4 = tail_weights()
    fe.firstconv = fe.layer1 = fe.layer3 = fe.lastconv = torch.nn.Identity()
    fe.layer2, fe.layer4 = torch.nn.Conv2d(4, 64, 1, bias=False), torch.nn.Conv2d(64, 128, 1, bias=False)
    with torch.no_grad():
        fe.layer2.weight.copy_(torch.from_numpy(w2)), fe.layer4.weight.copy_(torch.from_numpy(w4))
        full = fe.eval()(torch.from_numpy(tail_input())).numpy()
    assert full.shape == (1, 320, 64, 72)
    for k in (1, 2, 3, 4):
        out.update({f"tail.branch{k}.{n}": v.detach().numpy().copy() for n, v in getattr(fe, f"branch{k}").state_dict().items()})
    out["tail.rows"], out["tail.heads"] = np.array(TAIL_ROWS), np.array(TAIL_HEADS)
    out["tail.branches_out"] = full[:, 192:][:, :, list(TAIL_ROWS)].copy()
    out["tail.heads_out"] = full[:, list(TAIL_HEADS)][:, :, list(TAIL_ROWS)].copy()

    PATH = os.path.join(HERE, "psm_cases.npz")
    np.savez_compressed(PATH, **out)
    print("wrote", len(out), "arrays,", sum(a.size for a in out.values()), "cells,", os.path.getsize(PATH), "bytes")
