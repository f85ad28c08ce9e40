"""Golden vectors for a flow head whose convolutions run on the library's kernel, produced by running the REFERENCE's own
FlowHead.forward (models/raft_stereo/update.py:6-14) on the CPU (the tests read the recording, not the reference):

  * FlowHead(16, 32, 2): conv1 3x3 16 -> 32, ReLU, conv2 3x3 32 -> 2, one set of seeded weights;
  * "a": B = 2 on a 5x6 map;  "b": B = 2 on a 3x3 map.

Per case the input, conv1's output (a forward hook, before the ReLU) and the head's output; the two weights and biases once.
Arrays only.  BasicMotionEncoder has fixed channel counts and about 1 MB of weights, so it is not recorded.

Run:  python tests/golden/make_heads_golden.py REFERENCE_ROOT     (writes tests/golden/heads_cases.npz)
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
_oe = types.ModuleType("opt_einsum")          # imported by update.py, not used here
_oe.contract = torch.einsum
sys.modules.setdefault("opt_einsum", _oe)
warnings.filterwarnings("ignore")

import models.raft_stereo.update as UP  # noqa: E402

torch.manual_seed(6301)
rng = np.random.default_rng(6302)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))       # noqa: E731
head = UP.FlowHead(16, 32, 2).eval()
with torch.no_grad():
    for p in head.parameters():               # wider than the default initialisation: about half of conv1's outputs are cut by the ReLU
        p.mul_(2.0)
seen = {}
head.conv1.register_forward_hook(lambda m, i, o: seen.__setitem__("conv1", o.detach().clone()))
out = {f"{cv}_{p}": getattr(getattr(head, cv), p).detach().numpy().copy() for cv in ("conv1", "conv2") for p in ("weight", "bias")}
for name, B, H, W in (("a", 2, 5, 6), ("b", 2, 3, 3)):
    x = t(np.tanh(rng.standard_normal((B, 16, H, W))))
    with torch.no_grad():
        y = head(x)
    out[f"{name}_x"], out[f"{name}_conv1_out"], out[f"{name}_out"] = x.numpy().copy(), seen["conv1"].numpy().copy(), y.numpy().copy()

PATH = os.path.join(HERE, "heads_cases.npz")
np.savez_compressed(PATH, **out)
print("wrote", len(out), "arrays,", sum(a.size for a in out.values()), "cells,", os.path.getsize(PATH), "bytes")
