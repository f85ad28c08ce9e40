"""Golden vectors for the pictures (utils.py:17-79), produced by running the REFERENCE's own utils.py (it cannot travel to the
GPU box).  OpenCV is not installed: utils.py is imported with a stub cv2 whose dilate asserts a 1x1 kernel and returns a
copy, so only dilation 0 and 1 are generated and nothing of OpenCV is guessed.

Inputs: every bin edge of _color_map_errors_kitti and its float32 neighbours on both sides, the same around float32(edge / 3)
for scale = 3 (all of whose quotients are exact) and around float32(edge / 19) for scale = 19 (none is: there the comparison in
double against the float64 quotient differs from one in float32), the 'bad k' thresholds 1..4 and their neighbours, NaN and +-inf in disp and in gt, valid / mask drawn from
{0, 1, 0.5, -1}, BGR both ways.

Run:  python tests/golden/make_viz_golden.py <directory of the reference>     (writes tests/golden/viz_cases.npz)
"""
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ["VPP_REFERENCE"]
HERE = os.path.dirname(os.path.abspath(__file__))

cv2 = types.ModuleType("cv2")


def _dilate(img, kernel):
    assert kernel.shape == (1, 1) and kernel[0, 0] == 1, "only the identity is generated here"
    return img.copy()


cv2.dilate = _dilate
sys.modules["cv2"] = cv2
sys.path.insert(0, REF)
import utils as R  # noqa: E402

H, W = 19, 23
rng = np.random.default_rng(2024)
f32 = np.float32


def around(v):
    v = f32(v)
    return [np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))]


edges = [0.1875, 0.375, 0.75, 1.5, 3, 6, 12, 24, 48]
special = [f32(0)] + [f32(np.nextafter(f32(0), f32(1)))]
for e in edges:
    special += around(e)
for e in edges:
    special += around(f32(e / 3))
    special += around(f32(e / 19))            # the float32 nearest to the double quotient and its neighbours
for k in (1, 2, 3, 4):
    special += around(k)
special += [f32(np.nan), f32(np.inf), f32(1e30), f32(100)]
special = np.array(special, f32)


def frame_of(values):
    """A frame whose first pixels are `values` and whose rest is random over the bins."""
    a = (rng.uniform(0, 1, H * W) ** 3 * 70).astype(f32)
    assert len(values) <= H * W
    a[:len(values)] = values
    return a.reshape(H, W)


def valid_of(n_special):
    v = rng.choice(np.array([0, 1, 0.5, -1], f32), H * W, p=[0.25, 0.45, 0.15, 0.15]).astype(f32)
    v[:n_special] = 1          # the edge values are drawn ...
    v[n_special:n_special + 8] = [0, 1, 0.5, -1, 0, 1, 0.5, -1]
    return v.reshape(H, W)


out = {"special": special}

# ---- color_error_image_kitti -----------------------------------------------------------------
errors = frame_of(special)
mask = valid_of(len(special))
mask2 = mask.copy()
mask2.reshape(-1)[:len(special):3] = 0     # ... and some of them masked
out["ce_errors"], out["ce_mask"], out["ce_mask2"] = errors, mask, mask2
n = 0
for scale in (1, 3, 19):
    for bgr in (True, False):
        for dil in (0, 1):
            for mname, m in (("none", None), ("mask", mask), ("mask2", mask2)):
                out[f"ce_out_s{scale}_b{int(bgr)}_d{dil}_{mname}"] = R.color_error_image_kitti(errors.copy(), scale=scale, mask=m, BGR=bgr,
                                                                                                dilation=dil)
                n += 1

# ---- guided_visualize ------------------------------------------------------------------------
gt = rng.uniform(1, 60, (H, W)).astype(f32)
err = frame_of(special).reshape(-1)
sign = rng.choice(np.array([-1, 1], f32), H * W)
# disp = gt + err does not land on the edges after rounding: put the exact values where gt is 0, and gt = 0 under them
gtf = gt.reshape(-1).copy()
gtf[:len(special)] = 0
disp = (gtf + sign * err).astype(f32)
disp[:len(special)] = special * sign[:len(special)]
k = len(special) + 8
for i, (dv, gv) in enumerate([(np.nan, 1), (1, np.nan), (np.inf, 1), (-np.inf, 1), (1, np.inf), (1, -np.inf), (np.inf, np.inf),
                              (np.nan, np.nan), (3e19, -3e19), (1e-30, 0)]):
    disp[k + i], gtf[k + i] = dv, gv
valid = valid_of(len(special))
valid.reshape(-1)[k:k + 10] = [1, 1, 1, 1, 0.5, -1, 1, 1, 1, 1]
# the same non-finite values once more, not drawn
disp[k + 10:k + 14] = [np.nan, np.inf, 1, 1]
gtf[k + 10:k + 14] = [1, 1, np.nan, np.inf]
valid.reshape(-1)[k + 10:k + 14] = 0
disp, gtf = disp.reshape(H, W), gtf.reshape(H, W)
out["gv_disp"], out["gv_gt"], out["gv_valid"] = disp, gtf, valid
with np.errstate(all="ignore"):
    for scale in (1, 3, 19):
        for dil in (0, 1):
            r = R.guided_visualize(disp.copy(), gtf.copy(), valid.copy(), scale=scale, dilation=dil)
            assert list(r) == ['bad 1.0', 'bad 2.0', 'bad 3.0', 'bad 4.0', 'avgerr', 'rms']
            out[f"gv_out_s{scale}_d{dil}"] = np.stack([r[key] for key in r])

path = os.path.join(HERE, "viz_cases.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes,", n, "colour cases")
