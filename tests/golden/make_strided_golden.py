"""Golden vectors for the convolution kernel at stride 2, produced by running the REFERENCE's own ResidualBlock.forward
(models/raft_stereo/extractor.py:6-60) on the CPU (the tests read the recording, not the reference):

  * ResidualBlock(16, 32, 'instance', stride=2): conv1 3x3 16 -> 32 at stride 2, conv2 3x3 32 -> 32, downsample[0] 1x1 16 -> 32 at
    stride 2, three InstanceNorm2d without parameters; one set of seeded weights;
  * x: B = 2 on a 9x13 map, so that both axes are odd and the last window reaches past the map.

The input, the state dict (key for key), conv1(x) and downsample[0](x) (forward hooks), the block's output, and, so that every
stage between them can be held to its own referee from recorded inputs alone, conv2's input and output.  Arrays only.

Run:  python tests/golden/make_strided_golden.py REFERENCE_ROOT     (writes tests/golden/strided_cases.npz)
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

REF = sys.argv[1]                             # root of a checkout of the reference
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
_oe = types.ModuleType("opt_einsum")          # imported by the package's update.py, not used here
_oe.contract = torch.einsum
sys.modules.setdefault("opt_einsum", _oe)
warnings.filterwarnings("ignore")

import models.raft_stereo.extractor as EX  # noqa: E402

torch.manual_seed(6601)
rng = np.random.default_rng(6602)
blk = EX.ResidualBlock(16, 32, 'instance', stride=2).eval()
with torch.no_grad():
    for p in blk.parameters():                # wider than the default initialisation: sums of order 1
        p.mul_(2.0)
seen = {}
blk.conv1.register_forward_hook(lambda m, i, o: seen.__setitem__("conv1_out", o.detach().clone()))


def _conv2(m, i, o):
    seen["conv2_in"], seen["conv2_out"] = i[0].detach().clone(), o.detach().clone()


blk.conv2.register_forward_hook(_conv2)
blk.downsample[0].register_forward_hook(lambda m, i, o: seen.__setitem__("down_out", o.detach().clone()))
x = torch.from_numpy(np.tanh(rng.standard_normal((2, 16, 9, 13))).astype(np.float32))
with torch.no_grad():
    y = blk(x.clone())
out = {k: v.detach().numpy().copy() for k, v in blk.state_dict().items()}
out["x"], out["out"] = x.numpy().copy(), y.numpy().copy()
out.update({k: v.numpy().copy() for k, v in seen.items()})

PATH = os.path.join(HERE, "strided_cases.npz")
np.savez_compressed(PATH, **out)
print("wrote", len(out), "arrays,", sum(a.size for a in out.values()), "cells,", os.path.getsize(PATH), "bytes")
