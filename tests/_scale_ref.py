"""numpy restatement of --iscale / --oscale (test.py:136-148, :247-248), written from DESIGN section 5 (rule 1) -- not from the
HIP code.  Rule 1 is OpenCV 4.x `cv2.resize(img, (w, h))` (INTER_LINEAR) for 8U as we read it; rules 2 and 4 are torch's own
expressions, which the tests run on the CPU instead of restating them (scale_hints, decimate, restore below)."""
import numpy as np

COEF = 2048  # INTER_RESIZE_COEF_SCALE


def scaled_hw(H, W, s):
    return H // s, W // s


def axis_table(n_in, n_out):
    """(s0, s1, w0, w1) per output index: source indices (the second clamped) and int16 weights cvRound(x * 2048)."""
    inv = float(n_out) / n_in
    scale = 1.0 / inv
    s0 = np.empty(n_out, np.int64)
    s1 = np.empty(n_out, np.int64)
    w0 = np.empty(n_out, np.int64)
    w1 = np.empty(n_out, np.int64)
    for d in range(n_out):
        f = np.float32((d + 0.5) * scale - 0.5)     # double expression, rounded to float
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= n_in - 1:
            s, f = n_in - 1, np.float32(0)
        s0[d], s1[d] = s, min(s + 1, n_in - 1)
        w0[d] = int(np.rint(np.float32(np.float32(1) - f) * np.float32(COEF)))   # np.rint: half to even, like cvRound
        w1[d] = int(np.rint(f * np.float32(COEF)))
    return s0, s1, w0, w1


def resize_u8(img, w, h):
    """cv2.resize(img, (w, h)) for uint8 [H, W] or [H, W, C] (rule 1)."""
    a = np.asarray(img)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[..., None]
    H, W, _ = a.shape
    sy0, sy1, b0, b1 = axis_table(H, h)
    sx0, sx1, a0, a1 = axis_table(W, w)
    s = a.astype(np.int64)
    ax0, ax1 = a0[None, :, None], a1[None, :, None]
    t0 = s[sy0][:, sx0] * ax0 + s[sy0][:, sx1] * ax1
    t1 = s[sy1][:, sx0] * ax0 + s[sy1][:, sx1] * ax1
    by0, by1 = b0[:, None, None], b1[:, None, None]
    out = (((by0 * (t0 >> 4)) >> 16) + ((by1 * (t1 >> 4)) >> 16) + 2) >> 2
    out = out.astype(np.uint8)
    return out[..., 0] if squeeze else out


def area_fast_2x(img):
    """OpenCV's INTER_AREA fast path at exactly 2x: (p00 + p01 + p10 + p11 + 2) >> 2."""
    a = np.asarray(img).astype(np.int64)
    H, W = a.shape[:2]
    h, w = H // 2, W // 2
    a = a[:2 * h, :2 * w]
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def scale_hints(hints, s):
    """test.py:147-148: F.interpolate(hints, scale_factor=1./s, mode='nearest') / s, and the same for validhints (not divided)."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(hints, np.float32))[None, None]
    return (F.interpolate(t, scale_factor=1. / s, mode='nearest') / s)[0, 0].numpy()


def decimate(valid, s):
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(valid, np.float32))[None, None]
    return F.interpolate(t, scale_factor=1. / s, mode='nearest')[0, 0].numpy()


def restore(d, iscale, oscale):
    """test.py:247-248 on the CPU."""
    import torch
    import torch.nn.functional as F
    if iscale != 1 and iscale / oscale != 1:
        t = torch.from_numpy(np.ascontiguousarray(d, np.float32))[None]
        return (F.interpolate(t.unsqueeze(0), scale_factor=iscale / oscale, mode='nearest').squeeze(0) * iscale / oscale)[0].numpy()
    return d


def scaled_shape(H, W, iscale, oscale):
    """(h, w, Ho, Wo): the shape the matcher runs at and the shape of the restored map (F.interpolate: floor(n * scale_factor))."""
    h, w = H // iscale, W // iscale
    if iscale != 1 and iscale / oscale != 1:
        f = iscale / oscale
        return h, w, int(np.floor(h * f)), int(np.floor(w * f))
    return h, w, h, w
