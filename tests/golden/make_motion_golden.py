"""Golden vectors for the motion encoder's front (motion_kernels.hip), produced by running the REFERENCE's own lines on the
CPU (the GPU tests read the recording, not the reference):

  * models/raft_stereo/corr.py:110-145 -- CorrBlock1D, constructor and __call__, num_levels = 4, radius = 4;
  * models/raft_stereo/update.py:64-82 -- a seeded BasicMotionEncoder's convc1 and convf1, each with its ReLU.

B = 2, H4 = 5, W2 = W3 = 19: level widths 19 / 9 / 4 / 2, a map lower than the 7x7 window.  The weights are widened as in
make_gru_golden.py (times 3), so that the ReLUs cut on both sides, and are stored with the arrays: the recording holds
coords, flow, the four levels, the lookup, relu(convc1(lookup)), relu(convf1(flow)) and the two convolutions' weights and
biases.  No coordinate is infinite or NaN: the reference converts such a position to an index, which is undefined.

Run:  python tests/golden/make_motion_golden.py REFERENCE_ROOT     (writes tests/golden/motion_cases.npz)
"""
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F

REF = sys.argv[1]                             # root of a checkout of the reference
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
_oe = types.ModuleType("opt_einsum")          # imported by update.py, not used here
_oe.contract = torch.einsum
sys.modules.setdefault("opt_einsum", _oe)
warnings.filterwarnings("ignore")

import models.raft_stereo.corr as RC  # noqa: E402
import models.raft_stereo.update as UP  # noqa: E402

B, D, H4, W = 2, 8, 5, 19
N = B * H4 * W
torch.manual_seed(5601)
enc = UP.BasicMotionEncoder(types.SimpleNamespace()).eval()
with torch.no_grad():
    for p in enc.parameters():
        p.mul_(3.0)

rng = np.random.default_rng(5602)
# features on a grid of 1/16: the GEMM is exact in float32 in any order (make_corr_golden.py)
f2 = (np.clip(np.round(rng.standard_normal((B, D, H4, W)) * 16), -64, 64) / 16).astype(np.float32)
f3 = (np.clip(np.round(rng.standard_normal((B, D, H4, W)) * 16), -64, 64) / 16).astype(np.float32)
directed = np.array([0.0, -0.0, W - 1, W - 0.5, -4.0, -5.0, W + 3.0, -0.25, 1e30, -1e30, 2.0, 3.5, -64.0, 8.0 * W], np.float32)
cx = rng.uniform(-3.0, W + 3.0, N).astype(np.float32)
whole = rng.random(N) < 0.2
cx[whole] = np.floor(cx[whole])
cx[rng.permutation(N)[:len(directed)]] = directed
coords = np.zeros((B, 2, H4, W), np.float32)
coords[:, 0] = cx.reshape(B, H4, W)
coords[:, 1] = rng.uniform(0, H4, (B, H4, W)).astype(np.float32)          # channel 1 is not read
flow = (rng.standard_normal((B, 2, H4, W)) * 3.0).astype(np.float32)

out = dict(coords=coords, flow=flow)
with torch.no_grad():
    blk = RC.CorrBlock1D(torch.from_numpy(f2), torch.from_numpy(f3), num_levels=4, radius=4)
    for i in range(4):
        out[f"level{i}"] = blk.corr_pyramid[i].numpy().reshape(N, -1).astype(np.float32)
    lookup = blk(torch.from_numpy(coords))
    out["lookup"] = lookup.numpy().astype(np.float32)
    out["cor1"] = F.relu(enc.convc1(lookup)).numpy().astype(np.float32)
    out["flo1"] = F.relu(enc.convf1(torch.from_numpy(flow))).numpy().astype(np.float32)
for name in ("convc1", "convf1"):
    out[f"{name}_weight"] = getattr(enc, name).weight.detach().numpy().astype(np.float32)
    out[f"{name}_bias"] = getattr(enc, name).bias.detach().numpy().astype(np.float32)
assert [out[f"level{i}"].shape[1] for i in range(4)] == [19, 9, 4, 2]

PATH = os.path.join(HERE, "motion_cases.npz")
np.savez_compressed(PATH, **out)
print("wrote", len(out), "arrays,", sum(a.size for a in out.values()), "cells,", os.path.getsize(PATH), "bytes")
