"""Golden vectors for the read-out kernels, produced by running the REFERENCE's own lines on the CPU (`.cuda` is
patched to the identity as in make_frontend_golden.py; the GPU tests read the recording, not the reference):

  * models/psmnet/psmnet.py:227-233 + submodule.py:115-128 -- PSMNet.forward with every layer before line 227
    stubbed so that a chosen cost3 arrives there (classif3 returns it, everything before returns zeros), training = False.
  * models/raft_stereo/raft_stereo.py:69-81 -- the unbound RAFTStereo.upsample_flow.

Per case the inputs and the reference's float32 output.

Run:  python tests/golden/make_readout_golden.py REFERENCE_ROOT     (writes tests/golden/readout_cases.npz)
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
torch.Tensor.cuda = lambda self, *a, **k: self
_oe = types.ModuleType("opt_einsum")          # imported by update.py, not used here
_oe.contract = torch.einsum
sys.modules.setdefault("opt_einsum", _oe)
warnings.filterwarnings("ignore")

import models.psmnet.psmnet as P  # noqa: E402
import models.raft_stereo.raft_stereo as RS  # noqa: E402

out = {}


def psm_case(tag, B, D4, H4, W4, maxdisp, H, W, rng, spread=3.0, plant=None):
    cost3 = (rng.standard_normal((B, 1, D4, H4, W4)) * spread).astype(np.float32)
    if plant is not None:
        plant(cost3)
    net = P.PSMNet.__new__(P.PSMNet)
    torch.nn.Module.__init__(net)
    net.maxdisp = maxdisp
    net.training = False
    zero = torch.zeros(())
    net.feature_extraction = lambda x: torch.zeros((B, 1, 1, 1))
    net.dres0 = lambda c: zero
    net.dres1 = lambda c: zero
    net.dres2 = net.dres3 = net.dres4 = lambda c, a, b: (zero, None, None)
    net.classif1 = net.classif2 = lambda c: zero
    net.classif3 = lambda c: torch.from_numpy(cost3)
    im = torch.zeros((B, 3, H, W))
    with torch.no_grad():
        pred = P.PSMNet.forward(net, im, im)
    assert pred.shape == (B, 1, H, W)
    out[f"psm_{tag}_cost3"] = cost3
    out[f"psm_{tag}_meta"] = np.array([maxdisp, H, W], np.int64)
    out[f"psm_{tag}_pred"] = pred[:, 0].numpy().astype(np.float32)


def steep(cost3):
    cost3[0, 0, :, 0, 0] = np.where(np.arange(cost3.shape[2]) % 2 == 0, 80.0, -80.0)
    cost3[0, 0, :, -1, -1] = 0.75


rng = np.random.default_rng(3301)
psm_case("a", 2, 12, 5, 7, 48, 20, 28, rng)                       # exact x4
psm_case("b", 1, 12, 5, 7, 50, 23, 30, rng)                       # a general scale
psm_case("c", 1, 6, 3, 4, 24, 12, 16, rng, plant=steep)           # logits of +-80, a flat pixel
psm_case("d", 1, 48, 2, 3, 192, 8, 12, rng, spread=6.0)           # D = 192


def raft_case(tag, N, D, H, W, n_downsample, rng):
    f = 2 ** n_downsample
    flow = (rng.standard_normal((N, D, H, W)) * 12).astype(np.float32)
    mask = (rng.standard_normal((N, 9 * f * f, H, W)) * 2.5).astype(np.float32)
    with torch.no_grad():
        up = RS.RAFTStereo.upsample_flow(None, torch.from_numpy(flow), torch.from_numpy(mask), n_downsample)
    assert up.shape == (N, D, f * H, f * W)
    out[f"raft_{tag}_flow"], out[f"raft_{tag}_mask"] = flow, mask
    out[f"raft_{tag}_meta"] = np.array([n_downsample], np.int64)
    out[f"raft_{tag}_up"] = up.numpy().astype(np.float32)


raft_case("a", 2, 2, 3, 5, 2, rng)
raft_case("b", 1, 1, 2, 65, 2, rng)
raft_case("c", 1, 2, 3, 4, 3, rng)
raft_case("d", 1, 1, 4, 3, 1, rng)
raft_case("e", 1, 1, 1, 1, 2, rng)

PATH = os.path.join(HERE, "readout_cases.npz")
np.savez_compressed(PATH, **out)
print("wrote", len(out), "arrays,", os.path.getsize(PATH), "bytes")
