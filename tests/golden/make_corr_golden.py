"""Golden vectors for the correlation pyramid and lookup, produced by running the REFERENCE's own CorrBlock1D
(models/raft_stereo/corr.py:110-183), constructor and __call__, on the CPU (`.cuda` is patched to the identity as in
make_frontend_golden.py; the GPU tests read the recording, not the reference).

Per shape (B, D, H, W) and with / without hints: the feature maps and hints, level 0 (the modulated volume), the four
pooled levels the constructor builds, the coordinates and the lookup.  No coordinate is infinite or NaN: the
reference converts such a position to an index, which is undefined.

Run:  python tests/golden/make_corr_golden.py REFERENCE_ROOT     (writes tests/golden/corr_cases.npz)
"""
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1]                             # root of a checkout of the reference
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
torch.Tensor.cuda = lambda self, *a, **k: self
_oe = types.ModuleType("opt_einsum")          # imported by update.py (package __init__), not used by corr.py
_oe.contract = torch.einsum
sys.modules.setdefault("opt_einsum", _oe)
import models.raft_stereo.corr as RC  # noqa: E402

SHAPES = {"a": (2, 8, 20, 68), "b": (1, 4, 9, 150), "c": (1, 3, 6, 523), "d": (1, 2, 4, 64)}


def half_is_a_signed_zero(levels):
    """Pairs with a negative sum whose half rounds to zero: IEEE gives -0 there, torch's CPU avg_pool2d +0 (on a GPU,
    where the reference runs, the division is IEEE's).  The sign of that zero is the one thing this CPU recording
    would get wrong, so arrays that hold such a pair are not recorded: the next seed is taken."""
    n = 0
    for lv in levels[:-1]:
        w = lv.shape[1] // 2
        s = (np.float32(0) + lv[:, 0:2 * w:2]) + lv[:, 1:2 * w:2]
        n += int(((s < 0) & (s / np.float32(2) == 0)).sum())
    return n


def record(tag, B, Dc, H, W, rng, out):
    H4, W4 = H // 4, W // 4
    N = B * H4 * W4
    # features on a grid of 1/16 in [-4, 4]: every product has 14 bits and a sum of Dc <= 8 of them 17, so the GEMM is
    # exact in float32 in whatever order a library adds, and level 0 before the modulation is the same bits on any device
    f2 = (np.clip(np.round(rng.standard_normal((B, Dc, H4, W4)) * 16), -64, 64) / 16).astype(np.float32)
    f3 = (np.clip(np.round(rng.standard_normal((B, Dc, H4, W4)) * 16), -64, 64) / 16).astype(np.float32)
    valid = (rng.random((B, 1, H, W)) < 0.5).astype(np.float32)
    hints = rng.uniform(0.5, 4 * W4 - 1, (B, 1, H, W)).astype(np.float32) * valid
    directed = np.array([0.0, -0.0, W4 - 1, W4 - 0.5, -4.0, -5.0, W4 + 3.0, -0.25, 1e30, -1e30, 2.0, 3.5], np.float32)
    cx = rng.uniform(-3.0, W4 + 3.0, N).astype(np.float32)
    whole = rng.random(N) < 0.2
    cx[whole] = np.floor(cx[whole])
    assert N >= len(directed)
    cx[rng.permutation(N)[:len(directed)]] = directed
    coords = np.zeros((B, 2, H4, W4), np.float32)
    coords[:, 0] = cx.reshape(B, H4, W4)
    coords[:, 1] = rng.uniform(0, H4, (B, H4, W4)).astype(np.float32)      # channel 1 is not read
    out[f"{tag}_f2"], out[f"{tag}_f3"], out[f"{tag}_hints"], out[f"{tag}_valid"], out[f"{tag}_coords"] = f2, f3, hints, valid, coords
    skipped = 0
    for with_hints in (False, True):
        args = (torch.from_numpy(hints), torch.from_numpy(valid)) if with_hints else ()
        blk = RC.CorrBlock1D(torch.from_numpy(f2), torch.from_numpy(f3), *args, num_levels=4, radius=4)
        assert len(blk.corr_pyramid) == 5
        key = f"{tag}_{'hints' if with_hints else 'plain'}"
        levels = [lv.numpy().reshape(N, -1).astype(np.float32) for lv in blk.corr_pyramid]
        skipped += half_is_a_signed_zero(levels)
        for i, lv in enumerate(levels):
            out[f"{key}_level{i}"] = lv
        out[f"{key}_lookup"] = blk(torch.from_numpy(coords)).numpy().astype(np.float32)
    return skipped


out = {}
for tag, (B, Dc, H, W) in SHAPES.items():
    for seed in range(4177, 4277):
        part = {}
        if record(tag, B, Dc, H, W, np.random.default_rng([seed, B, Dc, H, W]), part) == 0:
            break
    else:
        raise RuntimeError("no seed without a signed-zero half")
    print(tag, "seed", seed)
    out.update(part)

PATH = os.path.join(HERE, "corr_cases.npz")
np.savez_compressed(PATH, **out)
print("wrote", len(out), "arrays,", os.path.getsize(PATH), "bytes")
