"""Golden vectors for PSMNet's stride-1 3-D convolutions on the library's kernels, produced by running the REFERENCE's own modules
(models/psmnet/psmnet.py, submodule.py) on the CPU (the tests read the recording, not the reference):

  * dres1.*: the reference's own Sequential(convbn_3d(16, 16, 3, 1, 1), ReLU, convbn_3d(16, 16, 3, 1, 1)) -- dres1's structure -- on
    [2,16,3,9,13] in eval mode, with seeded BatchNorm3d running statistics and affine parameters and convolution weights scaled so
    that sums are of order 1.  Stored: the state dict (key for key), the input, and seq(x) + x.
  * hg.*: the reference's own hourglass(16) on [1,16,4,8,12], called as dres3 calls it, with presqu and postsqu given.  Its input,
    convolution weights and BatchNorm constants are the integer formulas of tests/_psm3d_ref.py (hourglass_input, hourglass_state),
    exact in float32, which the tests repeat: no weight is stored.  Stored: presqu, postsqu and the three outputs.

Arrays only.  Run:  python tests/golden/make_psm3d_golden.py REFERENCE_ROOT     (writes tests/golden/psm3d_cases.npz)
"""
import os
import sys
import warnings

import numpy as np
import torch

REF = sys.argv[1]                             # root of a checkout of the reference
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))     # tests/: the formulas live with the referee
warnings.filterwarnings("ignore")

import models.psmnet.psmnet as PM  # noqa: E402
import models.psmnet.submodule as SM  # noqa: E402

import _psm3d_ref as P3  # noqa: E402

if __name__ == "__main__":
    gen = torch.Generator().manual_seed(7801)
    rng = np.random.default_rng(7802)
    out = {}
    seq = torch.nn.Sequential(SM.convbn_3d(16, 16, 3, 1, 1), torch.nn.ReLU(inplace=True), SM.convbn_3d(16, 16, 3, 1, 1))
    P3.seed_module(seq, gen)
    x = torch.from_numpy(np.tanh(rng.standard_normal(P3.DRES1_SHAPE)).astype(np.float32))
    with torch.no_grad():
        y = seq(x.clone()) + x
    out.update({f"dres1.{k}": v.detach().numpy().copy() for k, v in seq.state_dict().items() if not k.endswith("num_batches_tracked")})
    out["dres1.x"], out["dres1.out"] = x.numpy().copy(), y.numpy().copy()

    hg = PM.hourglass(16)
    state = {k: torch.from_numpy(v) for k, v in P3.hourglass_state(16).items()}
    missing = hg.load_state_dict(state, strict=False)
    assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys), missing
    hg.eval()
    presqu = np.tanh(rng.standard_normal(P3.HG_SQU)).astype(np.float32)
    postsqu = np.tanh(rng.standard_normal(P3.HG_SQU)).astype(np.float32)
    with torch.no_grad():
        o, pre, post = hg(torch.from_numpy(P3.hourglass_input()), torch.from_numpy(presqu.copy()), torch.from_numpy(postsqu.copy()))
    assert tuple(o.shape) == P3.HG_SHAPE and tuple(pre.shape) == tuple(post.shape) == P3.HG_SQU
    out["hg.presqu"], out["hg.postsqu"] = presqu, postsqu
    out["hg.out"], out["hg.pre"], out["hg.post"] = o.numpy().copy(), pre.numpy().copy(), post.numpy().copy()

    PATH = os.path.join(HERE, "psm3d_cases.npz")
    np.savez_compressed(PATH, **out)
    print("wrote", len(out), "arrays,", sum(a.size for a in out.values()), "cells,", os.path.getsize(PATH), "bytes")
