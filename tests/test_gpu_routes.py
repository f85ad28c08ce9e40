"""Every kernel instantiation the rSGM hot path can pick, checked by name and by value.

ROUTES below is the written specification of which kernels the library runs in the default environment (no VPPX_VARIANT,
no VPPX_VERT), read off the dispatch code: rsgm_launch_paths (lanes per pixel x disparities per lane, exact or not, cost
source, u8 / u16 volumes), fused_layout_wanted + run_aggregation (the fused layout: W / E on we12 or the line kernel, the
lock-step vertical kernel with 8 or 16 pixels per wave) and rsgm_launch_sum_wta_lr -> launch_lr_d / launch_lr_t /
launch_lr_t2 / launch_trap (or, when that returns 1, sum_wta + wta_right_t).  Every row is run: Engine.last_routes() must
name exactly the row's kernels, and the disparities and patterns must equal the CPU oracle bit for bit.  The sweep then
runs a grid of tiny cases and fails on any route that is not in the table -- a new kernel variant needs a row here.

Penalties: alpha = 0 and p2min = gamma = P, so that P2max = P.  The three byte-width thresholds are 24 + P2max <= 255
(u8 path volumes: P <= 231), 4 (24 + P2max) <= 255 (SW4 in the 8-volume sum: P <= 39) and 3 (24 + P2max) <= 255 (the
fused layout: P <= 61)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5


def _pen(p2):
    return dict(p2min=p2, gamma=p2, alpha=0.0)


def paths(gw, dpl, exact, src, t, dirs="ff"):
    return f"paths<{gw},{dpl},{'exact' if exact else 'partial'},{src},{t},dirs={dirs}>"


def sum_lr(dpl, t, nv, sw4=False, fullw=False):
    """launch_lr_t2's instantiation.  FAST (the specialised decision code) comes with SW4 and byte volumes only, FULLW
    (whole tiles, no row-end tests) with FAST only, when Wp % T == 0.  T = 64, one spare ring slot, except at D = 256
    (DPL 16): T = 32 without it."""
    T, spare = (32, "nospare") if dpl == 16 else (64, "spare")
    fast = sw4 and t == "u8"
    return (f"sum_lr<{dpl},{t},{nv},{T},{spare},{'sw4' if sw4 else 'nosw4'},{'fast' if fast else 'general'},16,"
            f"{'fullw' if fast and fullw else 'partw'}>")


def fallback(dpl):
    return [f"sum_wta<{dpl},partial,u16>", "wta_right_t"]


def case(B, W, D, p2=35, guided=False, H=24):
    return dict(B=B, H=H, W=W, D=D, p2=p2, guided=guided)


# (id, kernels, smallest case that reaches them).  W = 128 is a whole number of 64-pixel tiles (FULLW), W = 112 is not.
ROUTES = [
    # ---- 8-path layout, census cost.  <4,16>: D <= 64; <8,16>: D <= 128; <16,12>: D <= 192 below 8 frames; <8,24>: D <= 192
    # from 8 frames on; <16,16>: D <= 256.  u8 needs D % 64 == 0 and 24 + P2max <= 255 (rsgm_paths_elem_bytes); a partial D
    # (D != GW * DPL) writes u16 and its sum falls back (launch_lr_d covers D = 64 / 128 / 192 / 256 only).
    ("census_4x16_exact_u8", [paths(4, 16, 1, "census", "u8"), sum_lr(4, "u8", 8, sw4=True, fullw=True)], case(1, 128, 64)),
    ("census_8x16_exact_u8", [paths(8, 16, 1, "census", "u8"), sum_lr(8, "u8", 8, sw4=True, fullw=True)], case(1, 128, 128)),
    ("census_16x12_exact_u8", [paths(16, 12, 1, "census", "u8"), sum_lr(12, "u8", 8, sw4=True, fullw=True)], case(1, 128, 192)),
    # (B >= 3 at D = 192 with P2max <= 61 is the fused layout: P2max = 100 keeps the eight paths)
    ("census_8x24_exact_u8", [paths(8, 24, 1, "census", "u8"), sum_lr(12, "u8", 8)], case(8, 112, 192, p2=100)),
    ("census_16x16_exact_u8", [paths(16, 16, 1, "census", "u8"), sum_lr(16, "u8", 8, sw4=True, fullw=True)], case(1, 128, 256)),
    ("census_4x16_exact_u16", [paths(4, 16, 1, "census", "u16"), sum_lr(4, "u16", 8)], case(1, 112, 64, p2=232)),
    ("census_8x16_exact_u16", [paths(8, 16, 1, "census", "u16"), sum_lr(8, "u16", 8)], case(1, 112, 128, p2=232)),
    ("census_16x12_exact_u16", [paths(16, 12, 1, "census", "u16"), sum_lr(12, "u16", 8)], case(1, 112, 192, p2=232)),
    ("census_8x24_exact_u16", [paths(8, 24, 1, "census", "u16"), sum_lr(12, "u16", 8)], case(8, 112, 192, p2=232)),
    ("census_16x16_exact_u16", [paths(16, 16, 1, "census", "u16"), sum_lr(16, "u16", 8)], case(1, 112, 256, p2=232)),
    ("census_4x16_partial", [paths(4, 16, 0, "census", "u16")] + fallback(4), case(1, 112, 40)),
    ("census_8x16_partial", [paths(8, 16, 0, "census", "u16")] + fallback(8), case(1, 112, 96)),
    ("census_16x12_partial", [paths(16, 12, 0, "census", "u16")] + fallback(12), case(4, 112, 160)),
    ("census_8x24_partial", [paths(8, 24, 0, "census", "u16")] + fallback(12), case(9, 112, 160)),
    ("census_16x16_partial", [paths(16, 16, 0, "census", "u16")] + fallback(16), case(1, 112, 224)),
    # ---- 8-path layout, guided (always u16 volumes; the sum never takes SW4: max_path_value 0)
    ("guided_4x16_exact", [paths(4, 16, 1, "guided", "u16"), sum_lr(4, "u16", 8)], case(1, 112, 64, guided=True)),
    ("guided_4x16_partial", [paths(4, 16, 0, "guided", "u16")] + fallback(4), case(1, 112, 40, guided=True)),
    ("guided_8x16_exact", [paths(8, 16, 1, "guided", "u16"), sum_lr(8, "u16", 8)], case(1, 128, 128, guided=True)),
    ("guided_8x16_partial", [paths(8, 16, 0, "guided", "u16")] + fallback(8), case(1, 112, 96, guided=True)),
    ("guided_16x12_exact", [paths(16, 12, 1, "guided", "u16"), sum_lr(12, "u16", 8)], case(1, 112, 192, guided=True)),
    ("guided_16x12_partial", [paths(16, 12, 0, "guided", "u16")] + fallback(12), case(4, 112, 160, guided=True)),
    # B = 8 and B = 9 at D = 192 and 160: a whole number of XCD rounds and not
    ("guided_8x24_exact_B8", [paths(8, 24, 1, "guided", "u16"), sum_lr(12, "u16", 8)], case(8, 112, 192, guided=True)),
    ("guided_8x24_exact_B9", [paths(8, 24, 1, "guided", "u16"), sum_lr(12, "u16", 8)], case(9, 128, 192, guided=True)),
    ("guided_8x24_partial_B8", [paths(8, 24, 0, "guided", "u16")] + fallback(12), case(8, 128, 160, guided=True)),
    ("guided_8x24_partial_B9", [paths(8, 24, 0, "guided", "u16")] + fallback(12), case(9, 112, 160, guided=True)),
    ("guided_16x16_exact", [paths(16, 16, 1, "guided", "u16"), sum_lr(16, "u16", 8)], case(1, 112, 256, guided=True)),
    ("guided_16x16_partial", [paths(16, 16, 0, "guided", "u16")] + fallback(16), case(1, 112, 224, guided=True)),
    # ---- fused layout (default from 3 frames on for D = 128 / 192, for every D once the batch fills the chip with groups of
    # the 16-pixel kernel; byte volumes with 3 (24 + P2max) <= 255).  W / E: we12<D / 16> at D = 128 / 192 / 256, the line
    # kernel with dirs = 0x11 at D = 64.  The vertical kernel: vert3<D / 8> (8 pixels per wave) or vert4<D / 4> (16).  The sum
    # adds 4 byte volumes, with SW4 (3 x max <= 255); D = 256 takes the trapezoid ring with spare slots.
    ("fused_we12_8_vert3", ["we12<8>", "vert3<16>", sum_lr(8, "u8", 4, sw4=True, fullw=True)], case(8, 128, 128)),
    ("fused_we12_8_vert3_partw", ["we12<8>", "vert3<16>", sum_lr(8, "u8", 4, sw4=True)], case(8, 112, 128)),
    ("fused_we12_12_vert3", ["we12<12>", "vert3<24>", sum_lr(12, "u8", 4, sw4=True)], case(8, 112, 192)),
    # 960-wide frames: 4 groups of the 16-pixel kernel per XCD at D = 192, so from 8 frames on the launch next to W / E is the
    # 16-pixel kernel; at D = 128 from 12 frames on
    ("fused_we12_12_vert4", ["we12<12>", "vert4<48>", sum_lr(12, "u8", 4, sw4=True, fullw=True)], case(9, 960, 192, H=32)),
    ("fused_we12_8_vert4", ["we12<8>", "vert4<32>", sum_lr(8, "u8", 4, sw4=True, fullw=True)], case(12, 960, 128, H=32)),
    ("fused_we12_16_vert4_trap", ["vert4<64>", "we12<16>", "sum_trap<16,64,spare>"], case(16, 960, 256, H=32)),
    # D = 64 is fused only when the batch fills a round of the 16-pixel kernel (40 frames of 960 columns)
    ("fused_line_we_vert4", [paths(4, 16, 1, "census", "u8", dirs="11"), "vert4<16>", sum_lr(4, "u8", 4, sw4=True, fullw=True)],
     case(40, 960, 64, H=32)),
    # ---- sum / WTA.  NV = 8, u8: SW4 up to P2max = 39 (FAST, FULLW by width), none from 40 on (general code, never FULLW)
    ("sum8_u8_sw4_fullw", [paths(4, 16, 1, "census", "u8"), sum_lr(4, "u8", 8, sw4=True, fullw=True)], case(1, 128, 64, p2=39)),
    ("sum8_u8_sw4_partw", [paths(4, 16, 1, "census", "u8"), sum_lr(4, "u8", 8, sw4=True)], case(1, 112, 64, p2=39)),
    ("sum8_u8_nosw4_w128", [paths(4, 16, 1, "census", "u8"), sum_lr(4, "u8", 8)], case(1, 128, 64, p2=40)),
    ("sum8_u8_nosw4_w112", [paths(4, 16, 1, "census", "u8"), sum_lr(4, "u8", 8)], case(1, 112, 64, p2=40)),
    ("sum8_u8_sw4_128_partw", [paths(8, 16, 1, "census", "u8"), sum_lr(8, "u8", 8, sw4=True)], case(1, 112, 128)),
    ("sum8_u8_nosw4_128", [paths(8, 16, 1, "census", "u8"), sum_lr(8, "u8", 8)], case(1, 112, 128, p2=40)),
    ("sum8_u8_sw4_192_partw", [paths(16, 12, 1, "census", "u8"), sum_lr(12, "u8", 8, sw4=True)], case(1, 112, 192)),
    ("sum8_u8_sw4_256_partw", [paths(16, 16, 1, "census", "u8"), sum_lr(16, "u8", 8, sw4=True)], case(1, 112, 256)),
    ("sum8_u8_nosw4_256", [paths(16, 16, 1, "census", "u8"), sum_lr(16, "u8", 8)], case(1, 112, 256, p2=40)),
    # the fallback from 8 frames on
    ("fallback_40_B8", [paths(4, 16, 0, "census", "u16")] + fallback(4), case(8, 112, 40)),
    ("fallback_96_B8", [paths(8, 16, 0, "census", "u16")] + fallback(8), case(8, 128, 96)),
    ("fallback_160_B9", [paths(8, 24, 0, "census", "u16")] + fallback(12), case(9, 128, 160)),
    ("fallback_224_B8", [paths(16, 16, 0, "census", "u16")] + fallback(16), case(8, 112, 224)),
]
TABLE = {r for _, rs, _ in ROUTES for r in rs}
# rows whose routes the tiny-frame sweep cannot reach (wide frames, many frames): their own rows are their only witnesses
WIDE_ONLY = {"vert4<16>", "vert4<32>", "vert4<48>", "vert4<64>", "we12<16>", "sum_trap<16,64,spare>", paths(4, 16, 1, "census", "u8", dirs="11"),
             sum_lr(4, "u8", 4, sw4=True, fullw=True)}


@pytest.fixture(scope="module")
def eng():
    from vppstereo_amd.engine import Engine
    return Engine()


_batches = {}


def _batch(B, H, W, seed=SEED):
    key = (B, H, W, seed)
    if key not in _batches:
        _batches[key] = synth.make_batch(B, H, W, 64, 0.05, seed=seed + 31 * B + W)
    return _batches[key]


def _valid(hints):
    return (hints > 0).astype(np.float32)


def _run(eng, c, seed=SEED, b=None):
    """One Engine.vpp_rsgm call of case c: (disparities, left pattern, right pattern, routes)."""
    import torch
    b = b if b is not None else _batch(c["B"], c["H"], c["W"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    lv = torch.empty(b["left"].shape, dtype=torch.uint8, device=eng.device)
    rv = torch.empty_like(lv)
    out = eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), l_vpp=lv, r_vpp=rv, seed=seed,
                       rsgm_kw=dict(dmax=c["D"], **_pen(c["p2"])), validhints=t(_valid(b["hints"])) if c["guided"] else None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lv.cpu().numpy(), rv.cpu().numpy(), eng.last_routes()


_patterns = {}


def _oracle_patterns(b, f, seed, key=None):
    if key is not None and key in _patterns:
        return _patterns[key]
    oracle.init_rand(seed + f)
    lo, ro = oracle.vpp(b["left"][f], b["right"][f], b["hints"][f])
    if key is not None:
        _patterns[key] = (lo, ro)
    return lo, ro


def _frames(B):
    return list(range(B)) if B <= 9 else [0, B // 2, B - 1]


def _jobs(c, lv, rv, frames, seed=SEED, b=None):
    """Asserts the patterns of the given frames; returns the oracle's compute_rsgm jobs for their disparities."""
    cached = b is None
    b = _batch(c["B"], c["H"], c["W"]) if cached else b
    jobs = []
    for f in frames:
        lo, ro = _oracle_patterns(b, f, seed, key=(c["B"], c["H"], c["W"], f, seed) if cached else None)
        assert np.array_equal(lv[f], lo) and np.array_equal(rv[f], ro), (c, f, "pattern")
        kw = dict(dmax=c["D"], **_pen(c["p2"]))
        if c["guided"]:
            kw.update(hints=b["hints"][f], validhints=_valid(b["hints"][f]))
        jobs.append((c, f, b["left"][f], lo, ro, kw))
    return jobs


def _compare(jobs, outs):
    """Runs the oracle (compute_rsgm holds no shared state: threads) and compares bit for bit; outs[i] is job i's frame."""
    with ThreadPoolExecutor(8) as ex:
        wants = list(ex.map(lambda j: oracle.compute_rsgm(j[2], j[3], j[4], **j[5]), jobs))
    for (c, f, *_), got, want in zip(jobs, outs, wants):
        bad = int(np.sum(~((want == got) | (np.isnan(want) & np.isnan(got)))))
        assert bad == 0, f"{c} frame {f}: {bad} pixels differ from the oracle"


def _check(c, out, lv, rv, frames, seed=SEED, b=None):
    _compare(_jobs(c, lv, rv, frames, seed, b), [out[f] for f in frames])


@pytest.mark.parametrize("rid,want,c", ROUTES, ids=[r[0] for r in ROUTES])
def test_route_table_row(eng, rid, want, c):
    out, lv, rv, got = _run(eng, c)
    assert sorted(got) == sorted(want), f"{rid}: launched {got}, the table says {want}"
    _check(c, out, lv, rv, _frames(c["B"]))


def test_route_table_is_consistent():
    assert len({r[0] for r in ROUTES}) == len(ROUTES)
    assert WIDE_ONLY <= TABLE
    for _, rs, _ in ROUTES:
        assert len(set(rs)) == len(rs)


SWEEP = [case(B, W, D, p2=p2, guided=g) for W in (112, 128) for B in (1, 8, 9) for D in range(8, 257, 8)
         for p2 in (17, 39, 40, 231, 232) for g in (False, True)]


def test_route_sweep_is_complete(eng):
    """Tiny frames over B, every D, the P2max values around the thresholds, guided or not: every route seen must be a row of
    the table, and every route of the table must be seen here or be one of the wide-frame rows.  One frame of every case
    (a different one from case to case) is compared with the oracle."""
    seen, jobs, outs = {}, [], []
    for i, c in enumerate(SWEEP):
        out, lv, rv, got = _run(eng, c)
        for r in got:
            assert r in TABLE, f"route {r} reached by case {c} is not covered; add it to the table"
            seen.setdefault(r, c)
        f = i % c["B"]
        jobs += _jobs(c, lv, rv, [f])
        outs.append(out[f])
    missing = TABLE - set(seen) - WIDE_ONLY
    assert not missing, f"table routes the sweep never reached: {sorted(missing)}"
    assert not (WIDE_ONLY & set(seen)), "a wide-frame route showed up on tiny frames: move it out of WIDE_ONLY"
    print(f"\n{len(SWEEP)} cases reached {len(seen)} routes: " + ", ".join(sorted(seen)))
    _compare(jobs, outs)


# ---- the thresholds: the route flips exactly between the two values, and both sides equal the oracle
EDGES = [
    # 24 + P2max <= 255: u8 / u16 path volumes
    (case(1, 112, 64, p2=231), [paths(4, 16, 1, "census", "u8"), sum_lr(4, "u8", 8)]),
    (case(1, 112, 64, p2=232), [paths(4, 16, 1, "census", "u16"), sum_lr(4, "u16", 8)]),
    (case(8, 112, 192, p2=231), [paths(8, 24, 1, "census", "u8"), sum_lr(12, "u8", 8)]),
    (case(8, 112, 192, p2=232), [paths(8, 24, 1, "census", "u16"), sum_lr(12, "u16", 8)]),
    # 4 (24 + P2max) <= 255: SW4 in the sum of eight byte volumes
    (case(1, 128, 128, p2=39), [paths(8, 16, 1, "census", "u8"), sum_lr(8, "u8", 8, sw4=True, fullw=True)]),
    (case(1, 128, 128, p2=40), [paths(8, 16, 1, "census", "u8"), sum_lr(8, "u8", 8)]),
    # 3 (24 + P2max) <= 255: the fused layout
    (case(8, 128, 128, p2=61), ["we12<8>", "vert3<16>", sum_lr(8, "u8", 4, sw4=True, fullw=True)]),
    (case(8, 128, 128, p2=62), [paths(8, 16, 1, "census", "u8"), sum_lr(8, "u8", 8)]),
]


@pytest.mark.parametrize("c,want", EDGES, ids=[f"B{c['B']}_D{c['D']}_P{c['p2']}" for c, _ in EDGES])
def test_threshold_edges(eng, c, want):
    out, lv, rv, got = _run(eng, c)
    assert sorted(got) == sorted(want), (c, got)
    _check(c, out, lv, rv, _frames(c["B"]))


# ---- the stage API: aggregate_SSE aggregates a given cost volume (COST_DSI) and materialises S (sum_wta, no WTA)
@pytest.mark.parametrize("D,want", [(64, [paths(4, 16, 1, "dsi", "u16"), "sum_wta<4,exact,u16>"]),
                                    (96, [paths(8, 16, 0, "dsi", "u16"), "sum_wta<8,partial,u16>"])])
def test_stage_api_aggregate_routes(D, want):
    from vppstereo_amd import _lib, pyrSGM
    H, W = 32, 64
    rng = np.random.default_rng(D)
    img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    dsi = rng.integers(0, 60, (H, W, D)).astype(np.uint16)
    So, Sg = np.zeros((H, W, D), np.uint16), np.zeros((H, W, D), np.uint16)
    oracle.aggregate_SSE(img, dsi, So, W, H, D, 11, 17, 0.5, 35)
    pyrSGM.aggregate_SSE(img, dsi, Sg, W, H, D, 11, 17, 0.5, 35)
    assert _lib.last_routes(_lib.load(), _lib.default_context().handle) == want
    assert np.array_equal(So, Sg), int((So != Sg).sum())


# ---- guided edges
def test_guided_dense_validhints_every_pixel_owns_a_row(eng):
    """validhints = 1 everywhere, also where the hint is 0: the row buffer and the row map are full."""
    import torch
    B, H, W, D = 3, 40, 96, 128
    b = synth.make_batch(B, H, W, D, 0.05, seed=44)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    vh = np.ones((B, H, W), np.float32)
    lv = torch.empty(b["left"].shape, dtype=torch.uint8, device=eng.device)
    rv = torch.empty_like(lv)
    out = eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), l_vpp=lv, r_vpp=rv, seed=2, rsgm_kw=dict(dmax=D),
                       validhints=t(vh))
    torch.cuda.synchronize()
    assert sorted(eng.last_routes()) == sorted([paths(8, 16, 1, "guided", "u16"), sum_lr(8, "u16", 8)])
    out, lv, rv = out.cpu().numpy(), lv.cpu().numpy(), rv.cpu().numpy()
    for f in range(B):
        oracle.init_rand(2 + f)
        lo, ro = oracle.vpp(b["left"][f], b["right"][f], b["hints"][f])
        assert np.array_equal(lv[f], lo) and np.array_equal(rv[f], ro), f
        want = oracle.compute_rsgm(b["left"][f], lo, ro, hints=b["hints"][f], validhints=vh[f], dmax=D)
        assert np.array_equal(out[f], want), f


def test_guided_hints_inf_nan_negative_and_huge(eng):
    """+inf, -inf, NaN, negative hints and 1e30 at valid pixels, through Engine.rsgm (the cost re-weighting alone; such
    hints are no input for the virtual pattern).  NaN: the reference's numba astype(uint16) of a NaN product is
    cvttsd2si's 0x80000000, i.e. 0 -- the oracle's cast and the kernel's (int) conversion both give 0."""
    import torch
    B, H, W, D = 2, 36, 100, 64
    b = synth.make_batch(B, H, W, D, 0.08, seed=12)
    rng = np.random.default_rng(3)
    h = b["hints"].copy()
    vh = _valid(h)
    on = np.argwhere(vh > 0)
    special = np.array([np.inf, -np.inf, np.nan, -3.5, -250.0, 1e30, -1e30], np.float32)
    pick = rng.permutation(len(on))[: 7 * 12]
    for k, i in enumerate(pick):
        h[tuple(on[i])] = special[k % len(special)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    out = eng.rsgm(t(b["left"]), t(b["left"]), t(b["right"]), hints=t(h), validhints=t(vh), dmax=D).cpu().numpy()
    assert sorted(eng.last_routes()) == sorted([paths(4, 16, 1, "guided", "u16"), sum_lr(4, "u16", 8)])
    for f in range(B):
        want = oracle.compute_rsgm(b["left"][f], b["left"][f], b["right"][f], hints=h[f], validhints=vh[f], dmax=D)
        assert np.array_equal(out[f], want), f


def test_guided_engine_rsgm_B9_D160(eng):
    import torch
    B, H, W, D = 9, 30, 120, 160
    b = synth.make_batch(B, H, W, D, 0.05, seed=19)
    vh = _valid(b["hints"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    out = eng.rsgm(t(b["left"]), t(b["left"]), t(b["right"]), hints=t(b["hints"]), validhints=t(vh), dmax=D).cpu().numpy()
    assert sorted(eng.last_routes()) == sorted([paths(8, 24, 0, "guided", "u16")] + fallback(12))
    with ThreadPoolExecutor(8) as ex:
        wants = list(ex.map(lambda f: oracle.compute_rsgm(b["left"][f], b["left"][f], b["right"][f], hints=b["hints"][f],
                                                          validhints=vh[f], dmax=D), range(B)))
    for f in range(B):
        assert np.array_equal(out[f], wants[f]), f


# ---- guided memory-budget parts (VPPX_GUIDED_PART_MB is read when a context is created: a fresh child process)
_PB, _PH, _PW, _PD = 8, 32, 64, 192   # one frame's eight u16 volumes: 32 x 64 x 192 x 16 B = 6 MiB; 20 MiB hold 3 frames
_PARTS_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, synth
from vppstereo_amd.engine import Engine
B, H, W, D = %d, %d, %d, %d
b = synth.make_batch(B, H, W, D, 0.05, seed=61)
eng = Engine()
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
vh = t((b["hints"] > 0).astype(np.float32))
out = eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), g_occ="occlusion_heuristic", seed=9, rsgm_kw=dict(dmax=D), validhints=vh)
torch.cuda.synchronize()
print("vpp_rsgm parts", eng.last_call_parts(), "routes", ";".join(eng.last_routes()))
np.save(sys.argv[2], out.cpu().numpy())
out = eng.rsgm(t(b["left"]), t(b["left"]), t(b["right"]), hints=t(b["hints"]), validhints=vh, dmax=D)
torch.cuda.synchronize()
print("rsgm routes", ";".join(eng.last_routes()))
np.save(sys.argv[3], out.cpu().numpy())
""" % (_PB, _PH, _PW, _PD)


def test_guided_budget_parts_equal_one_part(eng, tmp_path):
    """With a 20 MiB budget 8 frames run as parts of 3: vpp_rsgm_parts makes 2 + 3 + 3 (the remainder is a part of its own,
    in front, as in every guided call -- an unguided call under VPPX_CHUNK=3 merges a remainder below 8 frames into a full
    part: 5 + 3), and vppx_rsgm_dev's loop 3 + 3 + 2.  Parts below 8 frames take <16,12> where the whole batch takes <8,24>:
    the routes show the split.  Both must equal the batch in one part bit for bit."""
    import torch
    b = synth.make_batch(_PB, _PH, _PW, _PD, 0.05, seed=61)
    vh_np = _valid(b["hints"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    vh = t(vh_np)
    whole_vr = eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), g_occ="occlusion_heuristic", seed=9,
                            rsgm_kw=dict(dmax=_PD), validhints=vh).cpu().numpy()
    assert eng.last_call_parts() == 1
    assert sorted(eng.last_routes()) == sorted([paths(8, 24, 1, "guided", "u16"), sum_lr(12, "u16", 8)])
    whole_r = eng.rsgm(t(b["left"]), t(b["left"]), t(b["right"]), hints=t(b["hints"]), validhints=vh, dmax=_PD).cpu().numpy()
    env = dict(os.environ, VPPX_GUIDED_PART_MB="20")
    d1, d2 = str(tmp_path / "vr.npy"), str(tmp_path / "r.npy")
    r = subprocess.run([sys.executable, "-c", _PARTS_CHILD, ROOT, d1, d2], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = {ln.split(" ")[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("vpp_rsgm", "rsgm"))}
    parted = ";".join([paths(16, 12, 1, "guided", "u16"), sum_lr(12, "u16", 8)])
    assert lines["vpp_rsgm"] == f"vpp_rsgm parts 3 routes {parted}", r.stdout
    assert lines["rsgm"] == f"rsgm routes {parted}", r.stdout
    assert np.array_equal(np.load(d1), whole_vr)
    assert np.array_equal(np.load(d2), whole_r)
    for f in (0, _PB - 1):
        g_occ = oracle.occlusion_heuristic(b["hints"][f])[1]
        oracle.init_rand(9 + f)
        lo, ro = oracle.vpp(b["left"][f], b["right"][f], b["hints"][f], g_occ=g_occ)
        want = oracle.compute_rsgm(b["left"][f], lo, ro, hints=b["hints"][f], validhints=vh_np[f], dmax=_PD)
        assert np.array_equal(whole_vr[f], want), f


# ---- the configuration tools/guided_bench.py times, at full size
def test_guided_benchmark_configuration_full_size(eng):
    """540 x 960 x 192, 16 frames, 3 % hints, the occlusion_heuristic mask: eight u16 path volumes of 3.2 GB each (past
    2^31 bytes), 25 GB together.  Frames 0, 7, 8 and 15 against the oracle."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * 2 ** 30:
        pytest.skip(f"needs 40 GiB of free device memory, {free / 2 ** 30:.1f} GiB free (the GPU is shared)")
    B, H, W, D = 16, 540, 960, 192
    b = synth.make_batch(B, H, W, D, 0.03, seed=1234)
    vh = _valid(b["hints"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    lv = torch.empty(b["left"].shape, dtype=torch.uint8, device=eng.device)
    rv = torch.empty_like(lv)
    out = eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), g_occ="occlusion_heuristic", l_vpp=lv, r_vpp=rv, seed=1,
                       rsgm_kw=dict(dmax=D), validhints=t(vh))
    torch.cuda.synchronize()
    assert eng.last_call_parts() == 1
    assert sorted(eng.last_routes()) == sorted([paths(8, 24, 1, "guided", "u16"), sum_lr(12, "u16", 8)])
    out, lv, rv = out.cpu().numpy(), lv.cpu().numpy(), rv.cpu().numpy()
    frames = (0, 7, 8, 15)
    pats = []
    for f in frames:
        g_occ = oracle.occlusion_heuristic(b["hints"][f])[1]
        oracle.init_rand(1 + f)
        lo, ro = oracle.vpp(b["left"][f], b["right"][f], b["hints"][f], g_occ=g_occ)
        assert np.array_equal(lv[f], lo) and np.array_equal(rv[f], ro), f
        pats.append((f, lo, ro))
    with ThreadPoolExecutor(4) as ex:
        wants = list(ex.map(lambda p: oracle.compute_rsgm(b["left"][p[0]], p[1], p[2], hints=b["hints"][p[0]],
                                                          validhints=vh[p[0]], dmax=D), pats))
    for (f, _, _), want in zip(pats, wants):
        assert np.array_equal(out[f], want), f
