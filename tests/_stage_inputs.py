"""Inputs and oracle references for the stage tests of the three fused kernels that have no pyrSGM-style stage of their
own (tests/test_gpu_stages.py): pad + gray + census in one launch (Engine.rsgm_front), the compact guided cost rows
(Engine.rsgm_guided_rows), median3x3 -> _linear_interpolate -> clip of both views (Engine.rsgm_mid).

A builder that misses the code it was written for tests nothing and says nothing, so every builder here checks what it
built against the oracle's own intermediates before it hands it out: `assert`s inside the builders, run without a GPU by
tests/test_stage_inputs_cpu.py and again by every GPU test that asks for a case.  Each case is built once per process
(lru_cache) and its arrays are read-only.

The geometry and the tile rule below restate the kernels' as a specification; nothing is imported from the library.
"""
import functools
import itertools

import numpy as np

import oracle
import synth


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def geom(H, W):
    """rsgm.py:254-260: (pad_t, pad_b, pad_l, pad_r, Hp, Wp)."""
    ph, pw = (16 - H % 16) % 16, (16 - W % 16) % 16
    return ph // 2, ph - ph // 2, pw // 2, pw - pw // 2, H + ph, W + pw


# ------------------------------------------------------------------------------------------------------------------ front
# pad_gray_census_kernel works on tiles of 64 x 16 padded pixels with a halo of 2: a tile at padded (x0, y0) = (64 bx, 16 by)
# reads the 68 x 20 padded rectangle from (x0 - 2, y0 - 2).  It takes the fast loader (unaligned dword loads straight from
# the frame) iff that rectangle maps into the un-padded frame without reflection, i.e. its source corner
# (x0 - 2 - pad_l, y0 - 2 - pad_t) is >= 0 and the rectangle ends inside W x H, and the tile's own 66 x 18 pixels lie inside
# the padded frame.  For bx, by >= 1 that is 62 - pad_l + 68 <= W and 14 - pad_t + 20 <= H at the first such tile.
FRONT_SHAPES = ((5, 5), (5, 17), (8, 8), (16, 16), (48, 144), (33, 129), (34, 131), (37, 203), (40, 160), (70, 330))
FRONT_NO_INTERIOR = FRONT_SHAPES[:4]
FRONT_KINDS = ("random", "two_level", "palette")


def interior_tiles(H, W):
    pt, _, pl, _, Hp, Wp = geom(H, W)
    n = 0
    for by in range(-(-Hp // 16)):
        for bx in range(-(-Wp // 64)):
            x0, y0 = 64 * bx, 16 * by
            sx0, sy0 = x0 - 2 - pl, y0 - 2 - pt
            n += sx0 >= 0 and sy0 >= 0 and sx0 + 68 <= W and sy0 + 20 <= H and x0 + 66 <= Wp and y0 + 18 <= Hp
    return n


def _plant_peaks(img, rng, lo, hi, n=3):
    """n windows of 5 x 5 pixels of `lo` with the centre `hi`: the centre's census code is 0xFFFFFF."""
    B, H, W, _ = img.shape
    if H < 9 or W < 9:
        return
    for f in range(B):
        for _ in range(n):
            y, x = int(rng.integers(2, H - 2)), int(rng.integers(2, W - 2))
            img[f, y - 2:y + 3, x - 2:x + 3] = lo
            img[f, y, x] = hi


def _front_image(rng, kind, B, H, W, C, which):
    if kind == "random":
        return rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    if kind == "two_level":
        # 100 / 101 in small blocks, every channel on its own: the strict `<` of the census is decided by ties, and for
        # C = 3 the gray value by the rounding of three weights
        bh, bw = ((2, 3), (3, 2), (1, 4))[which]
        lv = rng.integers(0, 2, (B, -(-H // bh), -(-W // bw), C), dtype=np.uint8)
        img = (100 + np.repeat(np.repeat(lv, bh, axis=1), bw, axis=2)[:, :H, :W]).astype(np.uint8)
        _plant_peaks(img, rng, 100, 101)
        return np.ascontiguousarray(img)
    assert kind == "palette" and C == 3
    ext = np.array([0, 1, 254, 255], np.uint8)
    a, b = ((1, 7), (3, 5), (5, 11))[which]
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.empty((B, H, W, 3), np.uint8)
    for f in range(B):
        idx = (a * xx + b * yy + 9 * f + which) % 64   # the 64 combinations of channel extremes, tiled over the frame
        img[f] = np.stack([ext[idx & 3], ext[(idx >> 2) & 3], ext[idx >> 4]], axis=-1)
    _plant_peaks(img, rng, 0, 255)
    return img


def front_reference(img):
    """(gray, census) of the padded frames of img [B,H,W,C], with the oracle's pieces in the order of compute_rsgm."""
    B, H, W, C = img.shape
    pt, pb, pl, pr, Hp, Wp = geom(H, W)
    gray = np.empty((B, Hp, Wp), np.uint8)
    cen = np.empty((B, Hp, Wp), np.uint32)
    for f in range(B):
        p = oracle.pad_reflect(img[f], pt, pb, pl, pr)
        gray[f] = oracle.rgb2gray(p) if C == 3 else p[..., 0]
        oracle.census5x5_SSE(np.ascontiguousarray(gray[f]), cen[f], Wp, Hp)
    return gray, cen


@functools.lru_cache(maxsize=None)
def front_case(H, W, C, B, kind):
    """dict(left, left_vpp, right_vpp: uint8 [B,H,W,C]; gray_left: uint8 [B,Hp,Wp]; census_l, census_r: uint32 [B,Hp,Wp];
    interior: number of tiles that take the fast loader)."""
    n_int = interior_tiles(H, W)
    assert (n_int == 0) == ((H, W) in FRONT_NO_INTERIOR), (H, W, n_int)
    rng = np.random.default_rng([H, W, C, B, FRONT_KINDS.index(kind)])
    imgs = [_front_image(rng, kind, B, H, W, C, k) for k in range(3)]
    for a, b in itertools.combinations(imgs, 2):   # a swapped image set must show in every frame
        assert all(not np.array_equal(a[f], b[f]) for f in range(B))
    gray_left = front_reference(imgs[0])[0]
    cens = [front_reference(im)[1] for im in imgs[1:]]
    for cen in cens:
        border = np.ones(cen.shape, bool)
        border[:, 2:-2, 2:-2] = False
        assert not cen[border].any()
        if n_int:
            inner = cen[:, 2:-2, 2:-2]
            assert (inner >> 23 & 1).any() and (inner & 1).any() and (inner == 0).any() and (inner == 0xFFFFFF).any(), (H, W, C, B, kind)
    return dict(left=_ro(imgs[0]), left_vpp=_ro(imgs[1]), right_vpp=_ro(imgs[2]), gray_left=_ro(gray_left),
                census_l=_ro(cens[0]), census_r=_ro(cens[1]), interior=n_int)


def front_cases():
    return [(H, W, C, B) for (H, W) in FRONT_SHAPES for C in (1, 3) for B in (1, 3)]


def front_kinds(C):
    return FRONT_KINDS if C == 3 else FRONT_KINDS[:2]


# -------------------------------------------------------------------------------------------------------------------- mid
MID_SHAPES = ((16, 16), (32, 80), (16, 64), (16, 128), (48, 272), (16, 2320))
MID_DIRECTED = (16, 2320, 3)   # (Hp, Wp, B) of the case whose directed rows hold a gap of every length at every bit offset
GAP_LENGTHS = tuple(range(2, 17))   # xr - xl: 2 .. 14 may fill, 15 and 16 are wider than the reference's window
F32 = np.float32
NEAR3 = np.nextafter(F32(3), F32(0))   # the largest float32 below 3
# end values (left, right) of a directed gap; their difference is exact in float32 and so in the reference's float64
_PAIRS = (
    (F32(7.625), F32(7.625)),            # 0
    (F32(5.25), F32(6.875)),             # < 3, rising
    (F32(21.5), F32(19.125)),            # < 3, falling
    (F32(10.25), F32(13.25)),            # exactly 3: refused (the rule is |d| < 3)
    (F32(13.25), F32(10.25)),            # exactly -3
    (F32(1), F32(1) + NEAR3),            # the largest difference below 3: filled
    (F32(1) + NEAR3, F32(1)),
    (F32(30.5), F32(36.25)),             # far apart
)
assert float(_PAIRS[5][1]) - 1.0 == float(NEAR3) and float(NEAR3) < 3.0


def _hole_values(rng, n):
    """What WTA output looks like where it is invalid: -10, 0, and small negatives in (-0.5, 0)."""
    k = rng.integers(0, 3, n)
    small = -rng.uniform(0.001, 0.499, n)
    return np.where(k == 0, -10.0, np.where(k == 1, 0.0, small)).astype(F32)


def _valid_values(rng, n):
    return rng.uniform(4.0, 16.0, n).astype(F32)


def _random_rows(rng, Hp, Wp):
    """Runs of 1-5 valid pixels and gaps of 1-18 holes."""
    m = np.empty((Hp, Wp), F32)
    for y in range(Hp):
        x, hole = 0, bool(rng.integers(0, 2))
        while x < Wp:
            n = int(rng.integers(1, 19)) if hole else int(rng.integers(1, 6))
            n = min(n, Wp - x)
            m[y, x:x + n] = _hole_values(rng, n) if hole else _valid_values(rng, n)
            x, hole = x + n, not hole
    return m


class _Directed:
    """Lays gaps out along directed rows (rows 0 and Hp - 1, which the median copies through): at a cursor column c that holds a
    valid pixel it places a gap of a length L for which (L, c mod 64) has not been seen yet, else a filler pixel."""

    def __init__(self, rng):
        self.rng = rng
        self.need = {(L, r) for L in GAP_LENGTHS for r in range(64)}
        self.turn = 0

    def _pick(self, c, room):
        """A gap length for a gap whose left end is column c; it may use columns up to c + room."""
        fits = [L for L in GAP_LENGTHS if L <= room]
        if not fits:
            return 0
        want = [L for L in fits if (L, c % 64) in self.need]
        if want:
            return want[self.turn % len(want)]
        if self.need and room > 40:
            return 0   # a filler pixel moves the cursor to a bit offset that is still missing
        return fits[self.turn % len(fits)] if self.turn % 3 else 0

    def row(self, Wp, begin_holes, end_holes, first_gap=0):
        """begin_holes > 0: the row begins with that many holes, else a gap begins at column 0; end_holes > 0: the row
        ends in that many holes, else a gap's right end is column Wp - 1; first_gap: the length of the row's first gap, which
        gets end values less than 3 apart."""
        rng = self.rng
        row = _hole_values(rng, Wp)
        last_L = 0 if end_holes else (3 + self.turn % 9 if Wp >= 32 else 3)
        end = Wp - end_holes - last_L   # one past the last column of the body; the body ends in a valid pixel
        c = begin_holes
        assert c < end
        row[c] = _valid_values(rng, 1)[0]
        if first_gap:
            assert c + first_gap <= end - 1
            row[c], row[c + first_gap] = _PAIRS[1]
            self.need.discard((first_gap, c % 64))
            c += first_gap
            if c < end - 1:
                c += 1
                row[c] = _valid_values(rng, 1)[0]
        while c < end - 1:
            self.turn += 1
            L = self._pick(c, end - 1 - c)
            if L == 0:
                c += 1
                row[c] = _valid_values(rng, 1)[0]
                continue
            a, b = _PAIRS[self.turn % len(_PAIRS)]
            row[c], row[c + L] = a, b
            self.need.discard((L, c % 64))
            c += L
            if c < end - 1:   # the next gap gets end points of its own
                c += 1
                row[c] = _valid_values(rng, 1)[0]
        if last_L:
            a, b = _PAIRS[(self.turn + 1) % 3]
            row[c], row[Wp - 1] = a, b
        return row


def gaps(row):
    """(xl, xr) of every maximal run of holes (<= 0) of a row that has a valid pixel on both sides."""
    v = np.flatnonzero(row > 0)
    return [(int(a), int(b)) for a, b in zip(v[:-1], v[1:]) if b - a >= 2]


def mid_reference(m):
    """(median, median -> interpolate -> clip) of one map with the oracle's pieces."""
    Hp, Wp = m.shape
    med = np.empty_like(m)
    oracle.median3x3_SSE(np.ascontiguousarray(m), med, Wp, Hp)
    out = med.copy()
    oracle._linear_interpolate(out, 15, 3)
    return med, np.clip(out, 0, None)


@functools.lru_cache(maxsize=None)
def mid_case(Hp, Wp, B):
    """dict(disp_l, disp_r: float32 [B,Hp,Wp]; med_l, med_r: the oracle's medians; ref_l, ref_r: the oracle's results;
    filled, refused: the number of gaps of at most 14 the reference filled / left alone)."""
    rng = np.random.default_rng([Hp, Wp, B])
    lay = _Directed(rng)
    disp = np.empty((2, B, Hp, Wp), F32)
    k = 0
    for f in range(B):
        for v in range(2):   # the two views differ in everything
            m = _random_rows(rng, Hp, Wp)
            for y in (0, Hp - 1):
                # (the widest gap the reference fills, once in every case: it is the one that needs the whole 27-bit window)
                m[y] = lay.row(Wp, begin_holes=(k % 2) * (1 + k % 5), end_holes=(k // 2 % 2) * (1 + k % 16 if Wp >= 32 else 1),
                               first_gap=14 if k == 2 else 0)
                k += 1
            disp[v, f] = m
    assert np.isfinite(disp).all()
    med, ref = np.empty_like(disp), np.empty_like(disp)
    for v in range(2):
        for f in range(B):
            med[v, f], ref[v, f] = mid_reference(disp[v, f])
    assert not np.array_equal(disp[0], disp[1])
    assert not np.array_equal(ref, np.clip(med, 0, None))
    # what the oracle did with every gap of its own median output
    filled = refused = 0
    seen, notes = set(), set()
    for v in range(2):
        for f in range(B):
            for y in range(Hp):
                mrow, rrow = med[v, f, y], ref[v, f, y]
                directed = y in (0, Hp - 1)
                if directed:
                    assert np.array_equal(mrow, disp[v, f, y])
                    lead = int(np.argmax(mrow > 0))
                    trail = int(np.argmax(mrow[::-1] > 0))
                    if lead:
                        notes.add("begins_in_holes")
                        assert not rrow[:lead].any()      # they stay holes, clipped to 0
                    if trail:
                        notes.add("ends_in_holes")
                        assert not rrow[Wp - trail:].any()
                for xl, xr in gaps(mrow):
                    L = xr - xl
                    full = bool((rrow[xl + 1:xr] > 0).all())
                    assert full or not rrow[xl + 1:xr].any(), "a gap is filled as a whole or not at all"
                    assert not (full and L > 14)
                    if L > 14:
                        if directed:
                            seen.add((L, xl % 64))
                        continue
                    filled += full
                    refused += not full
                    if not directed:
                        continue
                    seen.add((L, xl % 64))
                    d = float(mrow[xr]) - float(mrow[xl])
                    assert full == (abs(d) < 3.0)
                    if xl == 0:
                        notes.add("first_hole_is_column_1")
                    if xr == Wp - 1:
                        notes.add("right_end_is_last_column")
                    if abs(d) == 3.0:
                        notes.add("refused_at_3" if d > 0 else "refused_at_-3")
                    if abs(d) == float(NEAR3):
                        notes.add("filled_below_3" if d > 0 else "filled_above_-3")
                    if d == 0:
                        notes.add("flat")
                    if full and 0 < abs(d) < 2.9:
                        notes.add("rising" if d > 0 else "falling")
                    if full and L == 14:
                        notes.add("filled_14")
                    if full:
                        notes.add("trigger_is_xl+1" if max(xl + 1, xr - 7) == xl + 1 else "trigger_is_xr-7")
    floor = 3 if (Hp, Wp) == (16, 16) else 20
    assert filled >= floor and refused >= floor, (Hp, Wp, B, filled, refused)
    assert "filled_14" in notes
    if (Hp, Wp, B) == MID_DIRECTED:
        missing = {(L, r) for L in GAP_LENGTHS for r in range(64)} - seen
        assert not missing, sorted(missing)[:8]
        assert notes >= {"begins_in_holes", "ends_in_holes", "first_hole_is_column_1", "right_end_is_last_column", "refused_at_3",
                         "refused_at_-3", "filled_below_3", "filled_above_-3", "flat", "rising", "falling", "trigger_is_xl+1",
                         "trigger_is_xr-7"}, notes
    return dict(disp_l=_ro(disp[0]), disp_r=_ro(disp[1]), med_l=_ro(med[0]), med_r=_ro(med[1]), ref_l=_ro(ref[0]), ref_r=_ro(ref[1]),
                filled=filled, refused=refused, seen=frozenset(seen), notes=frozenset(notes))


def mid_cases():
    return [(Hp, Wp, B) for (Hp, Wp) in MID_SHAPES for B in (1, 3)]


# ----------------------------------------------------------------------------------------------------------------- guided
GUIDED_SHAPES = ((24, 48), (21, 130), (34, 300))
GUIDED_D = (8, 40, 64, 192, 256)


def guided_cases():
    """(H, W, D, B, density in percent).  About 5 %: every D at every shape (D = 256 at the two smaller ones) and B; no
    hints at all: every shape and B at D = 64; every pixel a hint: the smallest shape, every D and B."""
    out = [(H, W, D, B, 5) for (H, W) in GUIDED_SHAPES for D in GUIDED_D for B in (1, 3) if D < 256 or (H, W) != GUIDED_SHAPES[2]]
    out += [(H, W, 64, B, 0) for (H, W) in GUIDED_SHAPES for B in (1, 3)]
    out += [(24, 48, D, B, 100) for D in GUIDED_D for B in (1, 3)]
    return out


def _guided_frame(H, W, D, density, frame):
    """(left, right, hints, validhints) of one frame: a synthetic pair, with one pixel whose census codes differ in all 24 bits
    at disparity 3 from its partner, and hints / validhints that disagree in every way rsgm.py:123 allows."""
    fr = synth.make_frame(H, W, D, 0.05, seed=1000 + H + D, frame=frame)
    left, right = fr["left"].copy(), fr["right"].copy()
    yc, xc = H // 2, W // 2
    left[yc - 2:yc + 3, xc - 2:xc + 3] = 50      # centre above all 24 neighbours: 0xFFFFFF
    left[yc, xc] = 200
    right[yc - 2:yc + 3, xc - 5:xc] = 200        # centre (xc - 3) below all: 0
    right[yc, xc - 3] = 50
    hints = fr["hints"].copy()                    # fractional ground-truth values at about 5 % of the pixels
    if density == 100:
        rng = np.random.default_rng([H, W, D, frame])
        hints = np.where(rng.random((H, W)) < 0.8, rng.uniform(0, D + 20, (H, W)), 0).astype(F32)
    valid = (hints > 0).astype(F32)
    if density == 100:
        valid[:] = 1
        valid[::3, ::2] = 0.5
    # (y, x, hint, validhints)
    spots = [(0, 0, 1000.0, 1), (0, W - 1, 2.5, 1), (H - 1, 0, 0.0, 1), (H - 1, W - 1, D + 3.5, 1),   # the frame's corners
             (yc, xc, 1000.0, 1e-30),    # far from every d: the row is 10 x the census costs, 240 at d = 3
             (1, 0, 1000.0, 1),          # column 0: d > pad_l takes InvalidDispCost, 160
             (2, 3, 3.0, 1),             # an integer hint: weight 0 at d = 3
             (4, 1, 1.5, 1e-30), (H - 1, W // 3, 0.0, 2.0), (5, W - 1, float(D), 1)]
    off = [(3, 5, 7.25, 0.0), (3, 6, 4.5, -1.0), (6, 2, 2.0, -1e-30)]   # a hint without its mask: not guided
    for y, x, h, v in spots + (off if density != 100 else []):
        hints[y, x], valid[y, x] = h, v
    if density == 0:
        valid = -np.abs(valid) * (np.arange(W) % 2)   # zeros and negatives; the hints stay
    return left, right, hints, valid.astype(F32)


@functools.lru_cache(maxsize=None)
def guided_case(H, W, D, B, density):
    """dict(census_l, census_r: uint32 [B,Hp,Wp] from the oracle; hints, validhints: float32 [B,H,W]; owner: bool [B,Hp,Wp],
    the padded pixels that own a row; ref_rows: uint16 [n, D], the oracle's re-weighted rows of those pixels in raster order)."""
    pt, pb, pl, pr, Hp, Wp = geom(H, W)
    fr = [_guided_frame(H, W, D, density, f) for f in range(B)]
    hints = np.stack([x[2] for x in fr])
    valid = np.stack([x[3] for x in fr])
    cl = front_reference(np.stack([x[0] for x in fr]))[1]
    cr = front_reference(np.stack([x[1] for x in fr]))[1]
    owner = np.zeros((B, Hp, Wp), bool)
    owner[:, pt:pt + H, pl:pl + W] = valid > 0
    ref_rows = []
    for f in range(B):
        dsi = np.empty((Hp, Wp, D), np.uint16)
        oracle.costMeasureCensus5x5_xyd_SSE(np.ascontiguousarray(cl[f]), np.ascontiguousarray(cr[f]), dsi, Wp, Hp, D)
        ph, pv = np.zeros((Hp, Wp), F32), np.zeros((Hp, Wp), F32)   # rsgm.py:266-267
        ph[pt:pt + H, pl:pl + W], pv[pt:pt + H, pl:pl + W] = hints[f], valid[f]
        g = oracle._guided_dsi(dsi, ph, pv)
        assert np.array_equal(g[~owner[f]], dsi[~owner[f]])
        ref_rows.append(g[owner[f]])
        if density:
            yc, xc = H // 2 + pt, W // 2 + pl
            assert owner[f, yc, xc] and dsi[yc, xc, 3] == 24 and g[yc, xc, 3] == 240
            if pl < D - 1:   # only then is there an un-padded pixel with a disparity beyond its column
                assert owner[f, 1 + pt, pl] and dsi[1 + pt, pl, D - 1] == 16 and g[1 + pt, pl, D - 1] == 160
    ref_rows = np.concatenate(ref_rows)
    n = int(owner.sum())
    assert n == int((valid > 0).sum()) == len(ref_rows)
    if density == 0:
        assert n == 0 and (hints > 0).any()
    else:
        assert (ref_rows == 0).any() and (ref_rows == 240).any()
        assert (ref_rows == 160).any() or pl >= D - 1
        assert ((valid > 0) & (hints == 0)).any() and (valid == F32(1e-30)).any() and (hints > D).any()
        assert (hints[valid > 0] % 1 != 0).any()
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            assert (valid[:, y, x] > 0).all()
        assert owner[:, :, :D].any()   # hint pixels in padded columns xp < D
    if density == 100:
        assert n == B * H * W
    else:
        assert ((valid <= 0) & (hints > 0)).any() and (valid < 0).any()
    return dict(census_l=_ro(cl), census_r=_ro(cr), hints=_ro(hints), validhints=_ro(valid), owner=_ro(owner), ref_rows=_ro(ref_rows),
                n=n, geom=(pt, pl, Hp, Wp))


# ------------------------------------------------------------------------------------------------------- the pipeline once
TIE = dict(H=40, W=160, D=64, C=3, B=2)


@functools.lru_cache(maxsize=None)
def tie_case():
    """One batch through the whole oracle and through its stage natives: dict(left, left_vpp, right_vpp: uint8 [B,H,W,3];
    raw_l, raw_r: float32 [B,Hp,Wp], matchWTA_SSE + subPixelRefine / matchWTARight_SSE of the aggregated volume; pad_l, pad_r:
    compute_rsgm's padded maps after median / interpolate / clip; final: compute_rsgm's result [B,H,W])."""
    H, W, D, B = TIE["H"], TIE["W"], TIE["D"], TIE["B"]
    pt, pb, pl, pr, Hp, Wp = geom(H, W)
    b = synth.make_batch(B, H, W, D, 0.04, seed=77)
    lv, rv = np.empty_like(b["left"]), np.empty_like(b["right"])
    raw = np.empty((2, B, Hp, Wp), F32)
    padded = np.empty((2, B, Hp, Wp), F32)
    final = np.empty((B, H, W), F32)
    for f in range(B):
        oracle.init_rand(5 + f)
        lv[f], rv[f] = oracle.vpp(b["left"][f], b["right"][f], b["hints"][f])
        final[f], padded[0, f], padded[1, f] = oracle.compute_rsgm(b["left"][f], lv[f], rv[f], dmax=D, return_padded=True)
        gl = front_reference(b["left"][f:f + 1])[0][0]
        cl = front_reference(lv[f:f + 1])[1][0]
        cr = front_reference(rv[f:f + 1])[1][0]
        dsi, S = np.empty((Hp, Wp, D), np.uint16), np.empty((Hp, Wp, D), np.uint16)
        oracle.costMeasureCensus5x5_xyd_SSE(np.ascontiguousarray(cl), np.ascontiguousarray(cr), dsi, Wp, Hp, D)
        oracle.aggregate_SSE(np.ascontiguousarray(gl), dsi, S, Wp, Hp, D, 11, 17, 0.5, 35)
        oracle.matchWTA_SSE(S, raw[0, f], Wp, Hp, D, 0.95)
        oracle.subPixelRefine(S, raw[0, f], Wp, Hp, D, 0)
        oracle.matchWTARight_SSE(S, raw[1, f], Wp, Hp, D, 0.95)
        for v in range(2):   # the stage natives and compute_rsgm are one oracle
            assert np.array_equal(mid_reference(raw[v, f])[1], padded[v, f])
    assert not np.array_equal(np.clip(raw, 0, None), padded)
    return dict(left=_ro(b["left"]), left_vpp=_ro(lv), right_vpp=_ro(rv), raw_l=_ro(raw[0]), raw_r=_ro(raw[1]), pad_l=_ro(padded[0]),
                pad_r=_ro(padded[1]), final=_ro(final))
