"""numpy restatement of the reference's pictures, written for the tests (never the code under test): utils.py:17-79
(color_error_image_kitti, guided_visualize), the colour-mapped map of test.py:325-326 / :343 with a caller-supplied table,
max_val of test.py:318, and cv2.dilate with a d x d box of ones.  tests/test_viz_cpu.py holds it to tests/golden/viz_cases.npz
(the reference's own output) byte for byte for dilation <= 1 and its dilation to a brute-force double loop."""
import numpy as np

KEYS = ('bad 1.0', 'bad 2.0', 'bad 3.0', 'bad 4.0', 'avgerr', 'rms')

# utils.py:4-15
COLOR_MAP = np.array([
    [0, 0.1875, 149, 54, 49],
    [0.1875, 0.375, 180, 117, 69],
    [0.375, 0.75, 209, 173, 116],
    [0.75, 1.5, 233, 217, 171],
    [1.5, 3, 248, 243, 224],
    [3, 6, 144, 224, 254],
    [6, 12, 97, 174, 253],
    [12, 24, 67, 109, 244],
    [24, 48, 39, 48, 215],
    [48, np.inf, 38, 0, 165]]).astype(float)


def dilate(img, d):
    """cv2.dilate(img, np.ones((d, d))) of an [H,W,C] uint8 picture: per channel the maximum over the offsets
    -(d//2) .. d-1-(d//2) in both axes (the anchor is d//2), pixels outside the frame ignored; d <= 1: a copy."""
    d = int(d)
    if d <= 1:
        return img.copy()
    H, W = img.shape[:2]
    a = d // 2
    lo, hi = a, d - 1 - a
    pad = np.zeros((H + d - 1, W + d - 1) + img.shape[2:], img.dtype)  # 0: the identity of a maximum of uint8
    pad[lo:lo + H, lo:lo + W] = img
    out = np.zeros_like(img)
    for ky in range(d):
        for kx in range(d):
            np.maximum(out, pad[ky:ky + H, kx:kx + W], out=out)
    return out


def dilate_brute(img, d):
    """The same by a double loop over the pixels (checks `dilate`)."""
    H, W, Cc = img.shape
    out = np.zeros_like(img)
    if d <= 1:
        return img.copy()
    for y in range(H):
        for x in range(W):
            for c in range(Cc):
                m = 0
                for dy in range(-(d // 2), d - (d // 2)):
                    for dx in range(-(d // 2), d - (d // 2)):
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < H and 0 <= xx < W:
                            m = max(m, int(img[yy, xx, c]))
                out[y, x, c] = m
    return out


def error_colors(errors, scale=1, mask=None, bgr=True, dilation=1):
    """utils.py:17-36 for one frame: float32 errors compared in double against float64 lo / scale, hi / scale."""
    errors = np.asarray(errors, np.float32)
    e = errors.reshape(-1).astype(np.float64)
    col = np.zeros((e.shape[0], 3), np.uint8)
    with np.errstate(invalid="ignore"):
        for row in COLOR_MAP:
            lo, hi = np.float64(row[0]) / scale, np.float64(row[1]) / scale
            col[np.logical_and(e >= lo, e <= hi)] = row[2:].astype(np.uint8)
    if mask is not None:
        col[np.asarray(mask).reshape(-1) == 0] = 0
    if not bgr:
        col = col[:, [2, 1, 0]]
    return dilate(np.ascontiguousarray(col.reshape(errors.shape + (3,))), dilation)


def guided_visualize(disp, gt, valid, scale=1, dilation=7):
    """utils.py:39-79 for one frame."""
    disp, gt, valid = (np.asarray(a, np.float32) for a in (disp, gt, valid))
    with np.errstate(invalid="ignore", over="ignore"):
        diff = disp - gt
        error = np.abs(diff)
        rms = np.sqrt(diff * diff)
    out = {}
    for k in (1, 2, 3, 4):
        bad = np.zeros(disp.shape + (3,), np.uint8)
        with np.errstate(invalid="ignore"):
            bad[error > np.float32(k)] = (49, 54, 149)
            bad[error <= np.float32(k)] = (165, 0, 38)
        bad[valid == 0] = 0
        out['bad %d.0' % k] = dilate(bad, dilation)
    out['avgerr'] = error_colors(error, scale, valid, True, dilation)
    out['rms'] = error_colors(rms, scale, valid, True, dilation)
    return out


def colorize(x, max_val, lut, dilation=0):
    """test.py:325: lut[uint8(clamp(x, 0, max_val) / max_val * 255)] in float32; index 0 where the reference's cast is
    undefined (NaN input, max_val not > 0, NaN quotient)."""
    x = np.asarray(x, np.float32)
    mv = np.float32(max_val)
    idx = np.zeros(x.shape, np.uint8)
    if mv > 0:
        with np.errstate(invalid="ignore"):
            q = np.minimum(np.maximum(x, np.float32(0)), mv) / mv * np.float32(255)
        ok = ~np.isnan(x) & ~np.isnan(q)
        idx[ok] = q[ok].astype(np.uint8)
    return dilate(np.asarray(lut, np.uint8)[idx], dilation)


def finite_max(x):
    """test.py:318: the maximum with +-inf replaced by -inf (NaN propagates, as torch's max)."""
    x = np.asarray(x, np.float32)
    return np.where(np.isinf(x), np.float32(-np.inf), x).max()
