"""Float64 referee and input builders for the hand-off kernels (handoff_kernels.hip, to_nchw_kernel).

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_handoff_ref_cpu.py holds the referee to the golden
arrays the reference's own code produced and to oracle/frontends.py, and asserts every coverage claim the GPU
file (tests/test_gpu_handoff_ref.py) relies on, on the very arrays the GPU file uploads.

What is float32 and what is float64.  Kernel and reference do every step but one in correctly rounded float32,
and the referee does those steps the same way: the nearest index with its float32 scale, hints * valid / 4,
x * v - h, d - h, the square and the division by two_w2 (0.125 or 2: a power of two, so the division is
exact).  The argument of exp() is therefore bit-identical to the device's.  exp() itself is taken in float64
of that float32 argument and rounded once; (1 - v) + (v * 10) * e and the product with the feature / the
correlation run in float32 again (`out`).  `out64` is the same quantity in float64 from the argument on, so a
test can tell "off by the exp" from "off by more", and `limit()` is the distance to `out64` that a float32
implementation whose exp is within `exp_ulps` of the true value can reach.

The v == 0 rule takes a switch: rule="reference" applies the arithmetic everywhere ((1 - 0) + (0 * 10) * e, NaN
when the hint under the invalid pixel is not finite, since hints * valid is NaN there); rule="library" leaves
such cells untouched, which is what include/vppx.h documents.
"""
from types import SimpleNamespace

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                      # unit round-off of float32
TINY = 2.0 ** -126                  # smallest normal float32
PSM_TWO_W2, RAFT_TWO_W2 = F32(0.125), F32(2.0)
VALUES_OF_V = (0.0, -0.0, 1.0, 0.5, 2.0, -1.0)      # -1: a valid map is not promised to be 0 / 1, and v < 0 is not v == 0


# ---------------------------------------------------------------------------------------------------
# the operations
# ---------------------------------------------------------------------------------------------------
def nearest_indices(n_in, n_out, scale_dtype=F32):
    """min(int(floor(dst * scale)), n_in - 1), scale = n_in / n_out, product and scale in `scale_dtype`
    (float32 is ATen's and the kernel's; float64 is there to look for shapes at which the two differ)."""
    scale = scale_dtype(n_in) / scale_dtype(n_out)
    idx = np.floor(np.arange(n_out, dtype=scale_dtype) * scale).astype(np.int64)
    return np.minimum(idx, n_in - 1)


def f32_f64_index_splits(limit=2048):
    """Every (n_in, dst) with n_in < limit, n_out = n_in // 4, at which the float32 and the float64 product pick
    different source pixels."""
    found = []
    for n_in in range(4, limit):
        a, b = nearest_indices(n_in, n_in // 4), nearest_indices(n_in, n_in // 4, F64)
        found += [(n_in, int(d)) for d in np.flatnonzero(a != b)]
    return found


def subsample(hints, valid, raft=False):
    """[B,1,H,W] x 2 -> (h, v) float32 [B,H//4,W//4]: h = hints * valid / 4, for RAFT x * v - that."""
    hints, valid = np.asarray(hints, F32), np.asarray(valid, F32)
    H, W = hints.shape[2:]
    iy, ix = nearest_indices(H, H // 4), nearest_indices(W, W // 4)
    with np.errstate(invalid="ignore"):
        h = hints[:, 0][:, iy][:, :, ix]
        v = valid[:, 0][:, iy][:, :, ix]
        h = (h * v) / F32(4)
        if raft:
            h = np.arange(W // 4, dtype=F32)[None, None, :] * v - h
    return h, v


def exp_argument(d, h, two_w2):
    """-(d - h)^2 / two_w2 in float32, every step rounded like __fsub_rn / __fmul_rn / __fdiv_rn."""
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.asarray(d, F32) - np.asarray(h, F32)
        return (-(diff * diff)) / F32(two_w2)


def _modulate(c, v, arg, rule, exp):
    """c, v, arg broadcast to one shape.  -> (out float32, out64, e64, mod64)."""
    assert rule in ("reference", "library")
    assert c.dtype == F32 and v.dtype == F32 and arg.dtype == F32
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        e64 = np.exp(arg.astype(F64))
        e32 = e64.astype(F32) if exp is None else np.asarray(exp(arg), F32)
        one_minus, v10 = F32(1) - v, v * F32(10)
        out = c * (one_minus + v10 * e32)                       # three float32 roundings behind the exp
        mod64 = one_minus.astype(F64) + v10.astype(F64) * e64
        out64 = c.astype(F64) * mod64
    assert out.dtype == F32
    if rule == "library":
        keep = np.broadcast_to(v == 0, out.shape)
        out = np.where(keep, np.broadcast_to(c, out.shape), out)
        out64 = np.where(keep, np.broadcast_to(c, out.shape).astype(F64), out64)
    return out, out64, np.broadcast_to(e64, out.shape), np.broadcast_to(mod64, out.shape)


def psm_plain(fl, fr, maxdisp):
    """The un-modulated concat volume [B,2C,maxdisp//4,H4,W4]: copies and zeros, exact."""
    fl, fr = np.asarray(fl, F32), np.asarray(fr, F32)
    B, C, H4, W4 = fl.shape
    D4 = maxdisp // 4
    cost = np.zeros((B, 2 * C, D4, H4, W4), F32)
    for i in range(min(D4, W4)):
        cost[:, :C, i, :, i:] = fl[:, :, :, i:]
        cost[:, C:, i, :, i:] = fr[:, :, :, :W4 - i]
    return cost


def psm_volume(fl, fr, maxdisp, hints=None, valid=None, rule="reference", exp=None):
    """-> namespace(out, out64, plain, e64, mod64, v, c, arg): the volume, its float64 twin, and per cell the
    float64 exp, the float64 factor, the sub-sampled valid, the un-modulated cell and the float32 argument of the
    exp (all of the volume's shape)."""
    plain = psm_plain(fl, fr, maxdisp)
    if hints is None:
        return SimpleNamespace(out=plain, out64=plain.astype(F64), plain=plain, e64=None, mod64=None, v=None, c=plain)
    h, v = subsample(hints, valid)
    d = np.arange(maxdisp // 4, dtype=F32)[None, :, None, None]
    arg = exp_argument(d, h[:, None], PSM_TWO_W2)                # [B,D4,H4,W4]
    vb = np.broadcast_to(v[:, None], arg.shape)
    out, out64, e64, mod64 = _modulate(plain, np.ascontiguousarray(vb)[:, None], arg[:, None], rule, exp)
    vv = np.broadcast_to(vb[:, None], out.shape)
    return SimpleNamespace(out=out, out64=out64, plain=plain, e64=e64, mod64=mod64, v=vv, c=plain,
                           arg=np.broadcast_to(arg[:, None], out.shape))


def raft_modulate(corr, hints, valid, rule="reference", exp=None):
    """corr [B,H4,W2,1,W3] -> namespace like psm_volume's (plain = c = corr)."""
    corr = np.asarray(corr, F32)
    W3 = corr.shape[4]
    h, v = subsample(hints, valid, raft=True)                    # [B,H4,W2]
    assert h.shape == corr.shape[:3], (h.shape, corr.shape)
    k = np.arange(W3, dtype=F32)[None, None, None, None, :]
    arg = exp_argument(k, h[..., None, None], RAFT_TWO_W2)
    vv = np.ascontiguousarray(np.broadcast_to(v[..., None, None], corr.shape))
    out, out64, e64, mod64 = _modulate(corr, vv, arg, rule, exp)
    return SimpleNamespace(out=out, out64=out64, plain=corr, e64=e64, mod64=mod64, v=vv, c=corr, target=h, arg=arg)


def ulp32(x):
    """The float32 unit in the last place at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x)).astype(F32)).astype(F64)


def limit(ref, exp_ulps):
    """Per cell, how far from `ref.out64` a float32 implementation may be whose exp() is within `exp_ulps` units in
    the last place of the true value where that is a normal float32, and anywhere in [0, 2^-126] where it is
    subnormal or underflows (a flushed result is legitimate).  Behind the exp stand three float32 roundings:
    t = (v * 10) * e, s = (1 - v) + t and c * s; 1 - v and v * 10 are exact for every v the cases use (asserted
    by the CPU test).  First order, with a 2^-10 relative allowance for the second-order terms and 2^-148 per
    rounding that may land in the subnormal range:
        |c| * (|v10| * err_e + U * |t| + U * |s|) + U * |c * s|
    For v = 1 and a normal exp this is below (2 * exp_ulps + 2) * U * |c * s| < (2 * exp_ulps + 2) ulp of the cell."""
    with np.errstate(invalid="ignore", under="ignore"):
        v10 = np.abs(ref.v.astype(F64) * 10.0)
        err_e = np.where(ref.e64 >= TINY, exp_ulps * ulp32(ref.e64), TINY)
        c = np.abs(ref.c.astype(F64))
        lim = c * (v10 * err_e + U * v10 * ref.e64 + U * np.abs(ref.mod64)) + U * np.abs(ref.out64)
        return lim * (1 + 2.0 ** -10) + 2.0 ** -148 * (1 + c)


def cell_classes(ref):
    """(normal, subnormal, zero): boolean masks of the modulated cells (v != 0) by the class of the float32 exp."""
    mod = ref.v != 0
    e32 = ref.e64.astype(F32)
    return mod & (ref.e64 >= TINY), mod & (ref.e64 < TINY) & (e32 > 0), mod & (e32 == 0)


def compare(got, ref, exp_ulps):
    """-> (worst ulp distance to ref.out over the normal cells, cells beyond limit(), cells with v == 0 whose bits
    are not the input's).  Cells whose referee value is NaN or infinite count as beyond unless the other side has the
    same class.  The ulp distance is the report; the other two are what a test asserts.  (For a finite
    hint the reference's c * 1 is c as well, so the golden arrays are held to the third count too.)"""
    got = np.asarray(got)
    assert got.dtype == F32 and got.shape == ref.out.shape
    normal, _, _ = cell_classes(ref)
    lim = limit(ref, exp_ulps)
    keep = ref.v == 0                                            # compared bit for bit below, under either rule
    fin = np.isfinite(ref.out64) & ~keep
    with np.errstate(invalid="ignore"):
        beyond = fin & ~(np.abs(got.astype(F64) - ref.out64) <= lim)
        dist = np.abs(got.astype(F64) - ref.out.astype(F64)) / ulp32(ref.out)
    worst = float(dist[normal & fin].max()) if (normal & fin).any() else 0.0
    # a modulated cell whose referee value is not finite (a NaN hint under v != 0) has no distance: the device's
    # cell must be of the same class (NaN, or the same infinity)
    odd = ~np.isfinite(ref.out64) & ~keep
    beyond |= odd & ~((np.isnan(got) & np.isnan(ref.out64)) | (got.astype(F64) == ref.out64))
    changed = keep & (got.view(np.uint32) != np.ascontiguousarray(np.broadcast_to(ref.plain, got.shape)).view(np.uint32))
    return worst, int(beyond.sum()), int(changed.sum())


def corr_whole(f2, f3, hints, valid, exp_ulps):
    """CorrBlock1D.corr through a float32 GEMM: -> (the float64 value of every cell, how far a float32 implementation may be
    from it).  A float32 dot product of Dc terms is within Dc * 2^-24 * sum |a_i * b_i| of the exact one in any order of
    summation; / sqrt(Dc) adds its rounding, the float32 sqrt's and the rounding of the cell handed to the modulation
    (3 * 2^-24 relative, 4 allowed); behind it the modulation's own limit (tests/test_gpu_handoff_ref.py states the same bound
    on the golden arrays).  hints None: the plain volume."""
    Dc = f2.shape[1]
    a, b = np.asarray(f2, F64), np.asarray(f3, F64)
    dot = np.einsum("aijk,aijh->ajkh", a, b)[:, :, :, None, :]
    mag = np.einsum("aijk,aijh->ajkh", np.abs(a), np.abs(b))[:, :, :, None, :]
    c64 = dot / np.sqrt(float(Dc))
    c_err = (Dc * U * mag) / np.sqrt(float(Dc)) + 4 * U * np.abs(c64)
    if hints is None:
        return c64, c_err
    whole = raft_modulate(c64.astype(F32), hints, valid, rule="library")
    keep = whole.v == 0
    factor = np.where(keep, 1.0, np.abs(whole.mod64))
    lim = np.where(keep, 0.0, limit(whole, exp_ulps)) + factor * c_err * (1 + 2.0 ** -10)
    return np.where(keep, c64, c64 * whole.mod64), lim


def kitti_decode(u16):
    """disp = u16 / 256 (exact in float32), valid = disp > 0."""
    d = np.asarray(u16, np.uint16).astype(F64) / 256.0
    assert np.array_equal(d.astype(F32).astype(F64), d)
    return d.astype(F32), (d > 0).astype(np.uint8)


def pfm_decode_bits(raw, height, width, channels, little_endian):
    """The payload as uint32 words [H, W * channels], rows flipped, byte-swapped if big-endian: bits, not floats,
    so NaN payloads compare."""
    w = np.frombuffer(bytes(raw), "<u4" if little_endian else ">u4").astype(np.uint32)
    return np.ascontiguousarray(w.reshape(height, width * channels)[::-1])


def to_nchw(img_u8, pad_multiple=32):
    """uint8 [B,H,W,C] -> float32 [B,C,Hq,Wq] = (float)(v / 255.) replicate-padded, lo = pad // 2."""
    B, H, W, C = img_u8.shape
    ph = (((H // pad_multiple) + 1) * pad_multiple - H) % pad_multiple
    pw = (((W // pad_multiple) + 1) * pad_multiple - W) % pad_multiple
    x = (img_u8.astype(F64) / 255.0).astype(F32).transpose(0, 3, 1, 2)
    return np.pad(x, ((0, 0), (0, 0), (ph // 2, ph - ph // 2), (pw // 2, pw - pw // 2)), mode="edge"), (ph, pw)


# ---------------------------------------------------------------------------------------------------
# input builders: the GPU file and the CPU file see the same arrays
# ---------------------------------------------------------------------------------------------------
def scatter_to_full(h4, v4, H, W, rng):
    """Full-resolution [B,1,H,W] hints / valid whose nearest sub-sampling is (4 * h4, v4).  Every pixel the
    sub-sampling does not read is a decoy: valid = 1 with a hint of its own, so an implementation that reads
    another source pixel (another scale, a missing clamp) gets another answer."""
    B, H4, W4 = h4.shape
    assert (H // 4, W // 4) == (H4, W4)
    iy, ix = nearest_indices(H, H4), nearest_indices(W, W4)
    hints = rng.uniform(1.0, 9.0, (B, 1, H, W)).astype(F32)
    valid = np.ones((B, 1, H, W), F32)
    hints[:, 0][:, iy[:, None], ix[None, :]] = (h4 * F32(4)).astype(F32)
    valid[:, 0][:, iy[:, None], ix[None, :]] = v4
    return hints, valid


def _cycle_v(n, rng, p_zero=0.25):
    """n values of v: every member of VALUES_OF_V first, then v = 1 mostly, zeros with p_zero."""
    v = np.where(rng.random(n) < p_zero, 0.0, 1.0).astype(F32)
    odd = rng.random(n) < 0.15
    v[odd] = rng.choice(np.array(VALUES_OF_V, F32), int(odd.sum()))
    k = min(n, len(VALUES_OF_V))
    v[:k] = np.array(VALUES_OF_V, F32)[:k]
    return v


# name: (B, H4, W2, W3, rH, rW, kind)     H = 4 * H4 + rH, W = 4 * W2 + rW
RAFT_CASES = {
    "w1":        (1, 1, 1, 1, 0, 0, "every"),           # nrows = 1: residue 1, the smallest call
    "w24_all":   (1, 3, 24, 24, 1, 2, "all_normal"),    # every cell's exp is a normal float32
    "w63":       (1, 2, 63, 63, 3, 1, "directed"),      # nrows = 126: residue 2; one trip, lane 63 idle
    "w64":       (1, 2, 64, 64, 2, 3, "directed"),      # residue 0; one full trip
    "w65":       (1, 3, 65, 65, 1, 0, "directed"),      # nrows = 195: residue 3; second trip of one lane
    "w65_narrow": (1, 2, 30, 65, 0, 3, "directed"),     # W2 < W3
    "w65_wide":  (1, 1, 70, 65, 3, 2, "directed"),      # W2 > W3: targets right of the last column by themselves
    "w128":      (1, 1, 128, 128, 2, 1, "directed"),
    "w130":      (2, 1, 130, 130, 1, 3, "directed"),    # two frames that differ
    "w240":      (1, 2, 240, 240, 3, 0, "directed"),    # RAFT-Stereo at 960 columns: four trips
    "w65_none":  (1, 2, 65, 65, 2, 2, "none"),          # no hint at all
    "w65_every": (1, 2, 65, 65, 0, 1, "every"),         # every pixel a hint
}


def raft_case(name):
    """-> namespace(corr, hints, valid, v4, B, H4, W2, W3, H, W).  "directed": row r of a frame aims at the
    target column x * v - h that the row's turn names: one in every 64-wide trip, three left of column 0, three
    right of the last column, the rest uniform over the row; v cycles through VALUES_OF_V."""
    B, H4, W2, W3, rH, rW, kind = RAFT_CASES[name]
    rng = np.random.default_rng([31, len(name), B, H4, W2, W3])
    H, W = 4 * H4 + rH, 4 * W2 + rW
    n = B * H4 * W2
    corr = rng.standard_normal((B, H4, W2, 1, W3)).astype(F32)
    v = _cycle_v(n, rng)
    if kind == "none":
        v[:] = 0
    elif kind in ("every", "all_normal"):
        v[:] = 1
    x = np.tile(np.arange(W2, dtype=F64), B * H4)
    tgt = rng.uniform(0, W3, n)
    if kind == "directed":
        trips = (W3 + 63) // 64
        plan = [64 * t + min(31, W3 - 1 - 64 * t) + 0.25 for t in range(trips)] + [-3.0, -0.5, -14.0, W3 + 2.0, W3 - 0.5, W3 + 13.0]
        on = np.flatnonzero(v != 0)
        assert len(on) >= len(plan)
        rng.shuffle(on)
        tgt[on[:len(plan)]] = plan
    elif kind == "all_normal":
        tgt = rng.uniform(W3 / 2 - 1, W3 / 2, n)                 # |k - target| <= 13 < 13.2 for every k of 24
    h4 = (x * v - tgt).astype(F32)                               # hint / 4; negative where the target lies right of x
    h4, v4 = h4.reshape(B, H4, W2), v.reshape(B, H4, W2)
    hints, valid = scatter_to_full(h4, v4, H, W, rng)
    return SimpleNamespace(name=name, corr=corr, hints=hints, valid=valid, v4=v4, B=B, H4=H4, W2=W2, W3=W3, H=H, W=W)


# name: (B, C, H4, W4, rH, rW, maxdisp, kind)
PSM_CASES = {
    "w1":       (1, 2, 24, 1, 0, 3, 8, "directed"),      # W4 < 4
    "w3":       (1, 2, 8, 3, 1, 2, 16, "directed"),     # D4 = 4 > W4 through the scalar kernel
    "w4_d8":    (2, 2, 3, 4, 2, 1, 32, "directed"),     # D4 = 8 > W4 = 4 through the vector kernel, two frames
    "w4_d1":    (1, 3, 6, 4, 3, 0, 4, "directed"),      # D4 = 1 (maxdisp 4)
    "w5_d1":    (1, 1, 5, 5, 0, 0, 7, "directed"),      # D4 = 1 (maxdisp 7), C = 1, scalar kernel
    "w8":       (1, 1, 5, 8, 1, 3, 48, "directed"),     # D4 = 12 > W4 = 8, C = 1: plane i cuts a vector at each position
    "w8_all":   (1, 2, 4, 8, 2, 2, 16, "all_normal"),   # every modulated cell's exp is a normal float32
    "w68":      (1, 2, 16, 68, 3, 1, 48, "directed"),   # 272 vectors: the vector kernel's second block
    "w5_tall":  (1, 1, 52, 5, 2, 3, 16, "directed"),    # 260 cells a plane: the scalar kernel's second block
    "w8_none":  (1, 2, 2, 8, 0, 1, 16, "none"),
    "w8_every": (1, 2, 2, 8, 1, 0, 16, "every"),
}


def psm_case(name, split=None):
    """-> namespace(fl, fr, hints, valid, v4, maxdisp, ...).  "directed": hints on a plane (h an integer), half-way
    between two, above maxdisp, the rest uniform over the planes plus a margin; v cycles through VALUES_OF_V.
    `split` = (W, dst) builds the sub-sampling case instead: one row, the width at which float32 and float64
    pick different source columns for `dst`."""
    if split is not None:
        B, C, H4, W4, rH, rW, maxdisp, kind = 1, 1, 1, split[0] // 4, 2, split[0] % 4, 8, "every"
    else:
        B, C, H4, W4, rH, rW, maxdisp, kind = PSM_CASES[name]
    rng = np.random.default_rng([37, len(name), B, C, H4, W4, maxdisp])
    H, W, D4 = 4 * H4 + rH, 4 * W4 + rW, maxdisp // 4
    n = B * H4 * W4
    fl = rng.standard_normal((B, C, H4, W4)).astype(F32)
    fr = rng.standard_normal((B, C, H4, W4)).astype(F32)
    v = _cycle_v(n, rng)
    h4 = rng.uniform(-1.0, D4 + 1.0, n)
    if kind == "none":
        v[:] = 0
    elif kind in ("every", "all_normal"):
        v[:] = 1
    if kind == "directed":
        plan = [0.0, 0.5, D4 + 0.75, D4 + 40.0, float(D4 - 1), D4 - 1.5 if D4 > 1 else 0.5, float(D4 // 2)]
        on = np.flatnonzero(v != 0)
        assert len(on) >= len(plan)
        rng.shuffle(on)
        h4[on[:len(plan)]] = plan
    elif kind == "all_normal":
        h4 = rng.uniform(0.7, D4 - 1.7, n)                       # D4 = 4: |i - h| <= 2.3 < 3.3 for every plane
    h4, v4 = h4.astype(F32).reshape(B, H4, W4), v.reshape(B, H4, W4)
    hints, valid = scatter_to_full(h4, v4, H, W, rng)
    return SimpleNamespace(name=name, fl=fl, fr=fr, hints=hints, valid=valid, v4=v4, maxdisp=maxdisp, B=B, C=C, H4=H4,
                           W4=W4, H=H, W=W, D4=D4)


def pfm_payload(rows, rowwords, seed):
    """uint32 words [rows, rowwords] of a PFM payload as the file holds them (before any swap): normal floats with
    NaNs (quiet and signalling bit patterns), both infinities, -0 and subnormals planted in every row."""
    rng = np.random.default_rng([41, rows, rowwords, seed])
    w = rng.standard_normal((rows, rowwords)).astype(F32).view(np.uint32).copy()
    special = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF], np.uint32)
    for y in range(rows):
        xs = rng.integers(0, rowwords, len(special))
        w[y, xs] = special
    w[0, 0], w[-1, -1] = special[1], special[2]
    return w


PFM_SHAPES = [(rows, rowwords) for rowwords in (255, 256, 257, 960, 2880) for rows in (1, 540)]
KITTI_VALUES = np.array([0, 1, 255, 256, 65535], np.uint16)
KITTI_SIZES = (0, 1, 255, 256, 257)


def kitti_samples(n):
    rng = np.random.default_rng([43, n])
    a = rng.integers(0, 65536, n, dtype=np.uint16)
    a[rng.random(n) < 0.3] = 0
    k = min(n, len(KITTI_VALUES))
    a[:k] = KITTI_VALUES[:k]
    return a


# name: (B, H, W, C, pad_multiple)
NCHW_CASES = {
    "no_pad":   (1, 32, 64, 3, 32),
    "odd_pad":  (2, 27, 35, 3, 32),      # pads 5 and 29: lo = 2 < hi = 3, lo = 14 < hi = 15
    "wide":     (1, 5, 259, 2, 32),      # Wq = 288 > 256: the second x-block
    "c1":       (2, 9, 33, 1, 32),
    "mult1":    (1, 7, 13, 3, 1),
}


def nchw_image(name):
    B, H, W, C, mult = NCHW_CASES[name]
    rng = np.random.default_rng([47, B, H, W, C])
    a = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    a.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)[:a.size]        # every level
    return a, mult
