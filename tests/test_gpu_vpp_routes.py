"""Every kernel the front stage can pick -- occlusion heuristic, virtual pattern projection, bilateral filling -- checked by
name and by value.

ROUTES below is the written specification of what occ_launch, vpp_launch and vpp_launch_bilateral_fill (vpp_kernels.hip)
launch in the default environment (no VPPX_VARIANT), read off their dispatch code.  Every row is run:
Engine.last_front_routes() must name exactly the row's kernels, and every output of the call -- the patterned pair, n_hints,
the mask, the filtered map -- must equal the CPU oracle bit for bit (the stage is integer and exact-order float64: no
tolerance anywhere).  The sweep then runs a grid of tiny cases and fails on any route that is not in the table: a new kernel
variant needs a row here.  The rSGM half has the same in test_gpu_routes.py; the two lists do not share names.

What the launchers decide on:

  occ_launch    occ_warp4 when W % 4 == 0 and the hint pointer is 16-byte aligned, else occ_warp.
                occ_test<NJ,PT>: rx' = rx // 2, ry' = ry // 2, window count (2 rx' + 1)(2 ry' + 2) -- an odd number times an even
                one -- against 64 / 128 / 192 / 256: NJ = 1 / 2 / 3 / 4, above that 0.  PT = 2 when the LDS budget is below
                12 KB, else 4.  occ_dmap when the filtered map is asked for.
  vpp_launch    rnd: compact<dist|plain>, hint_range with per_frame_range, rowscan, rand;
                l_bits<NW,ROWS>: NW = 1 / 3 / 5 / 7 for wsize 1-2 / 3-4 / 5-6 / 7-8, ROWS = 4 when B * H >= 4096 and the budget is
                at least 18 KB, else 1; l_heavy<NW> with a mask that does not discard; l_wide for wsize >= 9;
                r_rows<u16|u32,mode,seg>: u32 list entries for W > 2048; the launch order is
                  independent  no mask, or a mask with discard_occluded: mode 1
                  late         a mask, the original right image kept (every fused call): mode 3, the replaying L pass last
                  inplace      a mask, R patterned in place (the VPP-only entries): mode 2, the L passes, mode 1
                and the L side runs on the side stream (side) in the first two, when the fork is possible: without a mask, or when
                the original right image is kept; else on the launch stream (main).
                maxDistance: compact, rowscan, then maxdist_wave (direction != 0, rad = n + n_agg_y <= 15, 64 W <= 132 KB, i.e.
                W <= 2112), else maxdist_lds (2 (2 rad + 1) W <= 60 KB), else maxdist_global.
  bilateral     gray_ctx + bilateral_fill in front of either method with use_bilateral_patch.

The LDS budget (vpp_rsgm_one, from rsgm_sum_lds_bytes): a pipelined fused call runs its front stage next to the previous
call's sum / WTA kernel and gets what that kernel leaves of a CU's 160 KB, minus 512 bytes, when that is between 6 KB and
64 KB; every other call gets 64 KB.  The uniform ring takes (NT D (T + 2) + T) 2 bytes with T = 64, NT = (62 + D) // 64 + 2
below D = 256 and T = 32, NT = 9 at D = 256:

  dmax                         ring bytes   left over   budget
  8 .. 144                     <= 95168     >= 68160    64 KB
  152 / 160 / 168 / 176 / 184  100448 ..    62880 / 57600 / 52320 / 47040 / 41760   the same (*)
  192                          126848       36480       36480
  200 .. 248                   >= 158528    < 6 KB      64 KB
  256, 8 paths (uniform ring)  156736       6592        6592
  256, fused, trapezoid ring   154592       8736        64 KB: four waves of 125 VGPRs per SIMD leave no registers either
  (*) only the widths where r_rows would be cut change (u16 rows need 24 W + 16 bytes: W > 1739 at D = 184), none of the
      12 KB / 18 KB decisions; these D take the materialised sum, so the guess is a pessimistic one.  Not in the table.

So the budgets a default call can see are 64 KB, 36480 B, 6592 B and the five of (*); none lies in [12 KB, 18 KB), the only
range where PT = 4 would meet ROWS = 1 for budget reasons: that combination is unreachable (ROWS = 1 comes with PT = 4 only
through B * H < 4096), and l_bits<NW,4> never meets occ_test<NJ,2>.  The sweep proves it: such a name would have no row.
r_rows is cut when a row's 24 W + 16 bytes (u16 entries) pass the budget, into ceil(W / ((budget - 512) // 24)) segments:

  D = 192   36480 B: 1 | 2 segments at W = 1519 | 1520; 3 from W = 2049 on (u32 entries, 40 bytes a column: three parts of 683)
  D = 256    6592 B: 1 | 2 at W = 274 | 275 (24 x 274 + 16 is the budget exactly), 2 | 3 at W = 506 | 507 (parts of 253)

Three branches inside the kernels are picked by the data, not by the launcher: an R list that overflows its 8 entries (and
the column W - 1 that an un-interpolated target of -1 wraps to), pixels deferred to the second L pass, an empty work list.
The rows meant to reach them assert a witness computed from the inputs and the reference's index arithmetic
(vpp_core_opt.pyx:81-89: d0 = floor(g), d1 = ceil(g), d = round(g), targets x - d0 + xw and x - d1 + xw, or x - d + xw)."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle
import synth  # noqa: F401  (the helpers of test_gpu_routes draw their batches from it)
from test_gpu_routes import _batch, _oracle_patterns, _frames

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7

GRAMMAR = re.compile(r"^(occ_warp4|occ_warp|occ_test<[0-4],[24]>|occ_dmap|hint_range|compact<(dist|plain)>|rowscan|rand|"
                     r"l_bits<[1357],[14]>|l_heavy<[1357]>|l_wide|r_rows<(u16|u32),mode=[123],seg=[1-9][0-9]*>|"
                     r"vpp_order<(independent|late|inplace),(side|main)>|maxdist_(wave|lds|global)|gray_ctx|bilateral_fill)$")


# ---- names
def occ(nj, pt=4, warp4=True, dmap=False):
    return ["occ_warp4" if warp4 else "occ_warp", f"occ_test<{nj},{pt}>"] + (["occ_dmap"] if dmap else [])


def rr(t="u16", modes=(1,), seg=1):
    return [f"r_rows<{t},mode={m},seg={seg}>" for m in modes]


def rnd(order, lside, rside=None, dist=False, hrange=False):
    """A call of the rnd method: the hint compaction and the draws, the launch order, the L kernels, the R launches."""
    side = "main" if order == "inplace" or order == "independent,main" else "side"
    order = order.split(",")[0]
    return ((["hint_range"] if hrange else []) + [f"compact<{'dist' if dist else 'plain'}>", "rowscan", "rand",
                                                  f"vpp_order<{order},{side}>"] + lside + (rside if rside is not None else rr()))


def lb(nw, rows=1):
    return [f"l_bits<{nw},{rows}>"]


def lh(nw):
    return [f"l_bits<{nw},1>", f"l_heavy<{nw}>"]


def md(which, dist=False):
    return [f"compact<{'dist' if dist else 'plain'}>", "rowscan", f"maxdist_{which}"]


BIL = ["gray_ctx", "bilateral_fill"]


def case(entry, B, H, W, C=3, p=0.05, vpp=None, mask=None, occ=None, D=64, piped=False, dmap=False, misaligned=False,
         dens=None, witness=None):
    """entry: "fused" (Engine.vpp_rsgm: the original right image is kept), "vpp" (vppx_vpp_dev: in place, with n_hints),
    "occ" (the heuristic alone).  mask: None, "given" (30 % of the pixels), "free" (a mask that touches no hint), "heur" (fused:
    computed on the way, with the parameters `occ`).  piped: a pipelined engine, the call made twice back to back."""
    return dict(entry=entry, B=B, H=H, W=W, C=C, p=p, vpp=dict(vpp or {}), mask=mask, occ=dict(occ or {}), D=D, piped=piped,
                dmap=dmap, misaligned=misaligned, dens=dens, witness=witness)


# window counts (2 (rx // 2) + 1)(2 (ry // 2) + 2): the reachable ones nearest to the four thresholds, on both sides
WIN = {20: (5, 3), 64: (1, 62), 66: (10, 4), 72: (9, 7), 128: (1, 126), 130: (12, 8), 192: (2, 62), 194: (96, 0), 238: (17, 13),
       256: (1, 254), 258: (42, 4), 420: (21, 19)}


def win(n):
    rx, ry = WIN[n]
    assert (2 * (rx // 2) + 1) * (2 * (ry // 2) + 2) == n
    return dict(rx=rx, ry=ry)


MASKED = dict(c_occ=0.15)
PIPE256 = dict(D=256, piped=True)   # fewer than 6 frames at D = 256: eight paths, the uniform ring, 6592 bytes left
PIPE192 = dict(D=192, piped=True)   # 36480 bytes left

# (id, kernels, smallest case that reaches them)
ROUTES = [
    # ---- occlusion heuristic alone
    ("occ_warp_w50", occ(2, warp4=False), case("occ", 2, 20, 50, p=0.1)),
    ("occ_warp4_w52", occ(2), case("occ", 2, 20, 52, p=0.1)),
    ("occ_warp_w52_pointer_plus_4", occ(2, warp4=False), case("occ", 2, 20, 52, p=0.1, misaligned=True)),
    ("occ_test_1_4", occ(1), case("occ", 2, 20, 52, p=0.1, occ=win(20))),
    ("occ_test_3_4", occ(3), case("occ", 2, 20, 52, p=0.1, occ=win(130))),
    ("occ_test_4_4", occ(4), case("occ", 2, 20, 52, p=0.1, occ=win(238))),
    ("occ_test_0_4", occ(0), case("occ", 2, 20, 52, p=0.1, occ=win(420))),
    ("occ_dmap", occ(2, dmap=True), case("occ", 1, 24, 64, p=0.5, dmap=True)),
    ("occ_dmap_w50", occ(2, warp4=False, dmap=True), case("occ", 1, 24, 50, p=0.5, dmap=True)),
    # ---- the heuristic next to a D = 256 sum kernel (pipelined, 2 frames): 512 pixels per block
    ("occ_test_1_2", occ(1, 2) + rnd("late", lh(3), rr(modes=(3,))), case("fused", 2, 20, 52, p=0.1, mask="heur", occ=win(20), **PIPE256)),
    ("occ_test_2_2", occ(2, 2) + rnd("late", lh(3), rr(modes=(3,))), case("fused", 2, 20, 52, p=0.1, mask="heur", **PIPE256)),
    ("occ_test_3_2", occ(3, 2) + rnd("late", lh(3), rr(modes=(3,))), case("fused", 2, 20, 52, p=0.1, mask="heur", occ=win(130), **PIPE256)),
    ("occ_test_4_2", occ(4, 2) + rnd("late", lh(3), rr(modes=(3,))), case("fused", 2, 20, 52, p=0.1, mask="heur", occ=win(238), **PIPE256)),
    ("occ_test_0_2", occ(0, 2, warp4=False) + rnd("late", lh(3), rr(modes=(3,))),
     case("fused", 2, 20, 50, p=0.1, mask="heur", occ=win(420), **PIPE256)),
    # ---- L side, first pass: one row per block (few rows), four (4096 rows: 32 frames of 128 x 48)
    ("l_bits_1_1", rnd("independent", lb(1)), case("fused", 2, 24, 64, vpp=dict(wsize=1))),
    ("l_bits_3_1", rnd("independent", lb(3)), case("fused", 2, 24, 64)),
    ("l_bits_5_1", rnd("independent", lb(5)), case("fused", 2, 24, 64, vpp=dict(wsize=5))),
    ("l_bits_7_1", rnd("independent", lb(7)), case("fused", 2, 24, 64, vpp=dict(wsize=7))),
    ("l_bits_1_4", rnd("independent", lb(1, 4)), case("fused", 32, 128, 48, vpp=dict(wsize=1))),
    ("l_bits_3_4", rnd("independent", lb(3, 4)), case("fused", 32, 128, 48)),
    ("l_bits_5_4", rnd("independent", lb(5, 4)), case("fused", 32, 128, 48, vpp=dict(wsize=5))),
    ("l_bits_7_4", rnd("independent", lb(7, 4)), case("fused", 32, 128, 48, vpp=dict(wsize=7, uniform_color=1))),
    ("l_bits_3_4_masked", rnd("late", lb(3, 4) + ["l_heavy<3>"], rr(modes=(3,))),
     case("fused", 32, 128, 48, vpp=MASKED, mask="given", witness=dict(deferred="some"))),
    # ---- L side, second pass (a mask, occluded hints kept)
    ("l_heavy_1", rnd("late", lh(1), rr(modes=(3,))), case("fused", 2, 24, 64, vpp=dict(wsize=1, **MASKED), mask="given", witness=dict(deferred="some"))),
    ("l_heavy_3", rnd("late", lh(3), rr(modes=(3,))), case("fused", 2, 24, 64, vpp=MASKED, mask="given", witness=dict(deferred="some"))),
    ("l_heavy_5", rnd("late", lh(5), rr(modes=(3,))), case("fused", 2, 24, 64, vpp=dict(wsize=5, **MASKED), mask="given", witness=dict(deferred="some"))),
    ("l_heavy_7", rnd("late", lh(7), rr(modes=(3,))), case("fused", 2, 24, 64, vpp=dict(wsize=7, interpolate=0, **MASKED), mask="given",
                                                           witness=dict(deferred="some"))),
    ("l_heavy_empty_work_list", rnd("late", lh(3), rr(modes=(3,))), case("fused", 2, 24, 64, vpp=MASKED, mask="free", witness=dict(deferred="none"))),
    # ---- L side, wide windows
    ("l_wide_9", rnd("independent", ["l_wide"]), case("fused", 2, 24, 64, vpp=dict(wsize=9))),
    ("l_wide_15", rnd("independent", ["l_wide"]), case("fused", 1, 24, 64, C=1, vpp=dict(wsize=15, uniform_color=1))),
    ("l_wide_31", rnd("independent", ["l_wide"]), case("vpp", 1, 40, 64, p=0.01, vpp=dict(wsize=31))),
    ("l_wide_9_masked_late", rnd("late", ["l_wide"], rr(modes=(3,))), case("fused", 2, 24, 64, vpp=dict(wsize=9, **MASKED), mask="given")),
    ("l_wide_9_masked_inplace", rnd("inplace", ["l_wide"], rr(modes=(2, 1))), case("vpp", 2, 24, 64, vpp=dict(wsize=9, **MASKED), mask="given")),
    # ---- R side: the launch orders
    ("order_independent_vpp_alone", rnd("independent", lb(3)), case("vpp", 3, 24, 64)),
    ("order_late_heuristic_on_the_way", occ(2) + rnd("late", lh(3), rr(modes=(3,))), case("fused", 3, 24, 64, p=0.1, mask="heur")),
    ("order_inplace", rnd("inplace", lh(3), rr(modes=(2, 1))), case("vpp", 3, 24, 64, vpp=MASKED, mask="given", witness=dict(deferred="some"))),
    ("order_inplace_r2l_gray", rnd("inplace", lh(5), rr(modes=(2, 1))),
     case("vpp", 2, 24, 66, C=1, vpp=dict(wsize=5, direction=0, interpolate=0, **MASKED), mask="given", witness=dict(deferred="some"))),
    ("order_discard_fused", rnd("independent", lb(3)), case("fused", 2, 24, 64, vpp=dict(discard_occluded=1), mask="given")),
    ("order_discard_vpp_alone", rnd("independent,main", lb(3)), case("vpp", 2, 24, 64, vpp=dict(discard_occluded=1), mask="given")),
    # ---- R side: list entries of 16 / 32 bits
    ("r_rows_u16_w2048", rnd("independent", lb(3)), case("vpp", 1, 5, 2048, p=0.04)),
    ("r_rows_u32_w2049", rnd("independent", lb(3), rr("u32", seg=3)), case("vpp", 1, 5, 2049, p=0.04)),
    ("r_rows_u32_w3700_inplace", rnd("inplace", lh(3), rr("u32", (2, 1), seg=4)),
     case("vpp", 1, 5, 3700, C=1, p=0.04, vpp=MASKED, mask="given", witness=dict(deferred="some"))),
    # ---- R side: column segments next to the sum kernel
    ("r_rows_seg2_d256", rnd("independent", lb(3), rr(seg=2)), case("fused", 2, 16, 300, **PIPE256)),
    ("r_rows_seg2_d256_masked", rnd("late", lh(3), rr(modes=(3,), seg=2)),
     case("fused", 2, 16, 300, vpp=MASKED, mask="given", witness=dict(deferred="some"), **PIPE256)),
    ("r_rows_seg3_d256_masked", rnd("late", lh(3), rr(modes=(3,), seg=3)),
     case("fused", 2, 16, 520, vpp=MASKED, mask="given", witness=dict(deferred="some"), **PIPE256)),
    ("r_rows_seg2_d192", rnd("independent", lb(3), rr(seg=2)), case("fused", 1, 8, 1600, p=0.03, **PIPE192)),
    ("r_rows_seg3_d192_u32", rnd("independent", lb(3), rr("u32", seg=3)), case("fused", 1, 8, 2100, p=0.03, **PIPE192)),
    # ---- the R lists: more than 8 (hint, patch column) items on one right pixel, and at most 8
    ("r_list_overflow_dense", rnd("inplace", lh(3), rr(modes=(2, 1))),
     case("vpp", 1, 36, 90, p=1.0, vpp=MASKED, mask="given", witness=dict(rlist="over", deferred="some"))),
    ("r_list_overflow_dense_no_interp", rnd("late", lh(3), rr(modes=(3,))),
     case("fused", 1, 36, 90, p=1.0, vpp=dict(interpolate=0, **MASKED), mask="given", witness=dict(rlist="over", wrap=True, deferred="some"))),
    ("r_list_sparse", rnd("inplace", lh(3), rr(modes=(2, 1))),
     case("vpp", 1, 36, 90, p=0.03, vpp=MASKED, mask="given", witness=dict(rlist="fits", deferred="some"))),
    ("mixed_density_0_3_100", rnd("inplace", lh(3), rr(modes=(2, 1))),
     case("vpp", 3, 36, 90, dens=[0.0, 0.03, 1.0], vpp=MASKED, mask="given", witness=dict(dens=True))),
    # ---- distance patch
    ("compact_dist", rnd("independent", lb(7), dist=True), case("fused", 2, 24, 64, vpp=dict(wsize=7, use_distance_patch=1))),
    ("compact_dist_hint_range", rnd("independent", lb(7), dist=True, hrange=True),
     case("fused", 2, 24, 64, vpp=dict(wsize=7, use_distance_patch=1, per_frame_range=1))),
    # (an even wsize: patch_size - 1 = 2n + 1 in the radius of vpp_standalone.py:9 -- the sweep's first run found 2n there)
    ("compact_dist_wsize_4", rnd("independent", lb(3), dist=True, hrange=True),
     case("fused", 2, 24, 64, p=0.1, vpp=dict(wsize=4, use_distance_patch=1, per_frame_range=1))),
    ("compact_dist_wsize_8_masked", rnd("inplace", lh(7), rr(modes=(2, 1)), dist=True),
     case("vpp", 2, 24, 64, p=0.1, vpp=dict(wsize=8, use_distance_patch=1, **MASKED), mask="given")),
    ("maxdist_dist_wsize_6", md("wave", dist=True), case("vpp", 2, 24, 64, p=0.1, vpp=dict(method=1, wsize=6, use_distance_patch=1))),
    # ---- maxDistance
    ("maxdist_wave", md("wave"), case("fused", 2, 24, 64, vpp=dict(method=1))),
    ("maxdist_wave_masked", md("wave"), case("vpp", 2, 24, 64, vpp=dict(method=1, **MASKED), mask="given")),
    ("maxdist_lds_direction_0", md("lds"), case("fused", 2, 24, 64, vpp=dict(method=1, direction=0))),
    ("maxdist_lds_rad_16", md("lds"), case("vpp", 1, 40, 64, vpp=dict(method=1, wsize=3, wsize_agg_y=31))),
    ("maxdist_global_direction_0", md("global"), case("vpp", 1, 6, 6145, C=1, p=0.02, vpp=dict(method=1, direction=0))),
    ("maxdist_dist_hint_range", ["hint_range"] + md("wave", dist=True),
     case("fused", 2, 24, 64, vpp=dict(method=1, wsize=5, use_distance_patch=1, per_frame_range=1))),
    # ---- bilateral filling
    ("bilateral_c3", BIL + rnd("independent", lb(5)), case("fused", 2, 24, 64, vpp=dict(wsize=5, use_bilateral_patch=1))),
    ("bilateral_c1", BIL + rnd("independent", lb(7)), case("vpp", 2, 24, 64, C=1, vpp=dict(wsize=7, use_bilateral_patch=1))),
    ("bilateral_maxdist", BIL + md("wave"), case("fused", 1, 24, 64, vpp=dict(method=1, wsize=5, use_bilateral_patch=1, wsize_agg_x=17))),
]
TABLE = {r for _, rs, _ in ROUTES for r in rs}
# routes the tiny-case sweep cannot reach, with the reason: their own rows (and the edges below) are their only witnesses
ROW_ONLY = {
    **{f"l_bits<{nw},4>": "4096 rows per call" for nw in (1, 3, 5, 7)},
    **{r: "rows wider than 2048 columns" for r in rr("u32", seg=3) + rr("u32", (2, 1), seg=4)},
    **{r: "rows of 507 columns and more behind a D = 256 call" for r in rr(modes=(3,), seg=3)},
    "maxdist_global": "2 (2 rad + 1) W above 60 KB",
    "occ_dmap": "the filtered map is an output of the heuristic's own entry point only",
    **{f"occ_test<{nj},{pt}>": "the sweep keeps the default window" for nj in (0, 1, 3, 4) for pt in (2, 4)},
}


# ---- inputs, the calls, the oracle
_inputs_cache = {}


def _inputs(c):
    key = (c["B"], c["H"], c["W"], c["C"], c["p"], tuple(c["dens"] or ()), c["mask"])
    if key in _inputs_cache:
        return _inputs_cache[key]
    B, H, W, Cn = c["B"], c["H"], c["W"], c["C"]
    rng = np.random.default_rng([B, H, W, Cn, int(c["p"] * 1000)])
    left = rng.integers(0, 256, (B, H, W, Cn), dtype=np.uint8)
    right = rng.integers(0, 256, (B, H, W, Cn), dtype=np.uint8)
    hints = np.zeros((B, H, W), np.float32)
    for f in range(B):
        p = c["dens"][f] if c["dens"] else c["p"]
        m = rng.random((H, W)) < p
        hints[f][m] = rng.uniform(0.3, min(0.6 * W, 60.0), int(m.sum())).astype(np.float32)
        # hints hugging the left border: targets below 0, and x - round(g) = -1 with x - floor(g) = 0 (the wraparound)
        hints[f][:, :3][m[:, :3]] = rng.choice(np.array([0.5, 1.5, 2.49, 2.5, 3.0], np.float32), int(m[:, :3].sum()))
    mask = None
    if c["mask"] == "given":
        mask = (rng.random((B, H, W)) < 0.3).astype(np.uint8)
    elif c["mask"] == "free":
        mask = ((rng.random((B, H, W)) < 0.3) & (hints == 0)).astype(np.uint8)
    _inputs_cache[key] = dict(left=left, right=right, hints=hints, mask=mask)
    return _inputs_cache[key]


@pytest.fixture(scope="module")
def eng():
    from vppstereo_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def peng():
    from vppstereo_amd.engine import Engine
    e = Engine()
    e.set_pipeline(True)
    return e


def _vpp_kw(c, inp):
    kw = dict(c["vpp"])
    if kw.get("use_distance_patch") and not kw.get("per_frame_range"):   # one range for the batch, as a caller would pass it
        pos = inp["hints"][inp["hints"] > 0]
        kw.update(dmin=float(pos.min()), dmax=float(pos.max()))
    return kw


def _run(engine, c):
    """One call of case c: dict(l, r, n_hints, conf, dmap -- numpy arrays or None), front routes, rSGM routes."""
    import torch
    from vppstereo_amd import _lib
    inp = _inputs(c)
    B, H, W, Cn = c["B"], c["H"], c["W"], c["C"]
    dev = engine.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if c["misaligned"]:   # a view 4 bytes past a 16-byte boundary of a larger buffer
        buf = torch.zeros(B * H * W + 8, dtype=torch.float32, device=dev)
        hints = buf[1:1 + B * H * W].view(B, H, W)
        hints.copy_(t(inp["hints"]))
        assert hints.data_ptr() % 16 == 4 and hints.is_contiguous()
    else:
        hints = t(inp["hints"])
        assert hints.data_ptr() % 16 == 0
    got = dict(l=None, r=None, n_hints=None, conf=None, dmap=None)
    if c["entry"] == "occ":
        conf = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        if c["dmap"]:
            dmap = torch.empty((B, H, W), dtype=torch.float32, device=dev)
            op = _lib.occ_params(**c["occ"])
            engine._bind_stream()
            _lib.check(engine.lib.vppx_occlusion_heuristic_full_dev(engine.ctx.handle, B, H, W, C.c_void_p(hints.data_ptr()), op.rx, op.ry,
                                                                    op.l, op.g, op.th_conf, op.th_filter, C.c_void_p(dmap.data_ptr()),
                                                                    C.c_void_p(conf.data_ptr())))
            got["dmap"] = dmap.cpu().numpy()
        else:
            engine.occlusion_heuristic(hints, out=conf, **c["occ"])
        got["conf"] = conf.cpu().numpy()
    elif c["entry"] == "vpp":
        l, r = t(inp["left"]), t(inp["right"])
        nh = torch.full((B,), -1, dtype=torch.int64, device=dev)
        mask = t(inp["mask"]) if inp["mask"] is not None else None
        p = _lib.vpp_params(seed=SEED, **_vpp_kw(c, inp))
        engine._bind_stream()
        _lib.check(engine.lib.vppx_vpp_dev(engine.ctx.handle, C.byref(p), B, H, W, Cn, C.c_void_p(l.data_ptr()), C.c_void_p(r.data_ptr()),
                                           C.c_void_p(hints.data_ptr()), C.c_void_p(mask.data_ptr()) if mask is not None else None, None,
                                           C.c_void_p(nh.data_ptr())))
        got.update(l=l.cpu().numpy(), r=r.cpu().numpy(), n_hints=nh.cpu().numpy())
    else:
        L, R = t(inp["left"]), t(inp["right"])
        g_occ = occ_out = None
        if c["mask"] == "heur":
            g_occ = dict(c["occ"]) or "occlusion_heuristic"
            occ_out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        elif inp["mask"] is not None:
            g_occ = t(inp["mask"])
        for _ in range(2 if c["piped"] else 1):   # (pipelined: the second call runs behind the first one's sum / WTA kernel)
            lv = torch.empty((B, H, W, Cn), dtype=torch.uint8, device=dev)
            rv = torch.empty_like(lv)
            engine.vpp_rsgm(L, R, hints, g_occ=g_occ, occ_out=occ_out, l_vpp=lv, r_vpp=rv, seed=SEED, vpp_kw=_vpp_kw(c, inp),
                            rsgm_kw=dict(dmax=c["D"]))
        got.update(l=lv.cpu().numpy(), r=rv.cpu().numpy())
        if occ_out is not None:
            got["conf"] = occ_out.cpu().numpy()
    torch.cuda.synchronize()
    return got, engine.last_front_routes(), engine.last_routes()


def _oracle_frame(c, f):
    """Frame f of case c on the CPU: dict(l, r, n_hints, conf, dmap)."""
    inp = _inputs(c)
    H, W, Cn = c["H"], c["W"], c["C"]
    hints = inp["hints"][f]
    want = dict(l=None, r=None, n_hints=None, conf=None, dmap=None)
    occ_f = np.zeros((H, W), np.uint8)
    if c["entry"] == "occ" or c["mask"] == "heur":
        want["dmap"], want["conf"] = oracle.occlusion_heuristic(hints, **c["occ"])
        occ_f = want["conf"]
        if c["entry"] == "occ":
            return want
    elif inp["mask"] is not None:
        occ_f = inp["mask"][f]
    kw = _vpp_kw(c, inp)
    wsize = kw.get("wsize", 3)
    l, r = inp["left"][f].copy(), inp["right"][f].copy()
    filled = None
    if kw.get("use_bilateral_patch"):   # vpp_standalone.py:413-420
        gray = oracle.rgb2gray(l, bgr=True) if Cn == 3 else np.ascontiguousarray(l[..., 0])
        filled = oracle.bilateral_filling(hints, gray, (wsize - 1) // 2)
    dmin = dmax = 0.0
    n = 0
    if np.count_nonzero(hints):
        if kw.get("use_distance_patch"):
            pos = hints[hints > 0]
            dmin, dmax = (pos.min(), pos.max()) if kw.get("per_frame_range") else (np.float32(kw["dmin"]), np.float32(kw["dmax"]))
        common = (kw.get("direction", 1), kw.get("c", 0.4), kw.get("c_occ", 0.0), np.ascontiguousarray(occ_f != 0, np.uint8),
                  bool(kw.get("discard_occluded", 0)), bool(kw.get("interpolate", 1)), filled, bool(kw.get("use_distance_patch", 0)),
                  dmin, dmax, kw.get("distance_gamma", 0.3))
        oracle.init_rand(SEED + f)
        if kw.get("method", 0) == 1:
            n = oracle.virtual_projection_scan_max_dist(l, r, hints, W, H, Cn, bool(kw.get("uniform_color", 0)), wsize,
                                                        kw.get("wsize_agg_x", 64), kw.get("wsize_agg_y", 3), *common)
        else:
            n = oracle.virtual_projection_scan_rnd(l, r, hints, W, H, Cn, bool(kw.get("uniform_color", 0)), wsize, *common)
    want.update(l=l, r=r, n_hints=n)
    return want


def _check(c, got, frames):
    for f in frames:
        want = _oracle_frame(c, f)
        for k in ("l", "r", "conf", "dmap"):
            if got[k] is not None:
                assert want[k] is not None and np.array_equal(got[k][f], want[k]), (c, f, k, int((got[k][f] != want[k]).sum()))
        if got["n_hints"] is not None:
            assert int(got["n_hints"][f]) == want["n_hints"], (c, f, "n_hints")


# ---- witnesses of the branches the data picks: from the inputs and the reference's index arithmetic, never from the library
def _hint_items(c, f):
    """(hint row y, hint column x, occluded, [(window column xw the scan visits, its right targets, wrapped to W - 1)])."""
    inp = _inputs(c)
    kw = c["vpp"]
    g, W = inp["hints"][f], c["W"]
    occ_f = inp["mask"][f] if inp["mask"] is not None else np.zeros_like(g, np.uint8)
    n = (kw.get("wsize", 3) - 1) // 2
    for y, x in zip(*np.nonzero(g > 0)):
        v = float(g[y, x])
        d0, d1 = int(np.floor(v)), int(np.ceil(v))
        d = int(np.floor(v + 0.5))   # C's round() of a positive value
        cols = []
        for xw in range(-n, n + 1):
            if 0 <= x + xw <= W - 1 and 0 <= x - d0 + xw <= W - 1:
                if kw.get("interpolate", 1):
                    cols.append((xw, {x - d0 + xw} | ({x - d1 + xw} if 0 <= x - d1 + xw <= W - 1 else set()), False))
                else:
                    cols.append((xw, {(x - d + xw) % W}, x - d + xw == -1))   # -1 wraps to column W - 1
        yield int(y), int(x), bool(occ_f[y, x]), cols


def _witness(c):
    w, H, W = c["witness"], c["H"], c["W"]
    n = (c["vpp"].get("wsize", 3) - 1) // 2
    inp = _inputs(c)
    if w.get("dens"):
        share = [(inp["hints"][f] > 0).mean() for f in range(c["B"])]
        assert share[0] == 0.0 and 0.02 < share[1] < 0.04 and share[2] == 1.0, share
    load = np.zeros((c["B"], H, W), np.int64)
    deferred = np.zeros((c["B"], H, W), bool)
    wrapped = 0
    for f in range(c["B"]):
        for y, x, occluded, cols in _hint_items(c, f):
            y0, y1 = max(0, y - n), min(H - 1, y + n)
            for xw, targets, wraps in cols:
                for tx in targets:
                    load[f, y0:y1 + 1, tx] += 1
                wrapped += wraps
            if occluded:
                deferred[f, y0:y1 + 1, max(0, x - n):min(W - 1, x + n) + 1] = True
    if w.get("rlist") == "over":
        assert load.max() > 8, load.max()
    if w.get("rlist") == "fits":
        assert 0 < load.max() <= 8, load.max()
    if w.get("wrap"):
        assert wrapped > 0
    if w.get("deferred") == "some":
        assert deferred.sum() > 0
    if w.get("deferred") == "none":
        assert deferred.sum() == 0 and inp["mask"].sum() > 0


# ---- the table
@gpu
@pytest.mark.parametrize("rid,want,c", ROUTES, ids=[r[0] for r in ROUTES])
def test_front_route_table_row(eng, peng, rid, want, c):
    if c["witness"]:
        _witness(c)
    got, routes, _ = _run(peng if c["piped"] else eng, c)
    assert sorted(routes) == sorted(want), f"{rid}: launched {routes}, the table says {want}"
    _check(c, got, _frames(c["B"]))


def test_front_route_table_is_consistent():
    """Runs without a GPU: unique ids, no name twice in a row, every name well-formed."""
    assert len({r[0] for r in ROUTES}) == len(ROUTES)
    assert set(ROW_ONLY) <= TABLE, set(ROW_ONLY) - TABLE
    for rid, rs, c in ROUTES:
        assert len(set(rs)) == len(rs), rid
        for r in rs:
            assert GRAMMAR.match(r), (rid, r)
        assert c["entry"] in ("fused", "vpp", "occ") and c["mask"] in (None, "given", "free", "heur")
    for cs, rs in EDGES:
        for r in rs:
            assert GRAMMAR.match(r), r
    for n, (rx, ry) in WIN.items():
        assert (2 * (rx // 2) + 1) * (2 * (ry // 2) + 2) == n
    # the reachable window counts nearest to the thresholds: an odd number times an even one
    reach = {a * b for a in range(1, 400, 2) for b in range(2, 400, 2)}
    for th, (lo, hi) in {64: (64, 66), 128: (128, 130), 192: (192, 194), 256: (256, 258)}.items():
        assert max(v for v in reach if v <= th) == lo and min(v for v in reach if v > th) == hi


# ---- the sweep
def _sweep_cases():
    out = []
    grid = itertools.product((0, 1), range(1, 12), ("none", "discard", "keep"), ("fused", "vpp"))
    for i, (method, wsize, mask, entry) in enumerate(grid):
        h = (i * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF   # the other axes: mixed bits of the case number
        h = ((h ^ (h >> 15)) * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        bit = lambda k: (h >> k) & 1
        B = (1, 8, 33)[(h >> 12) % 3]
        W = (44, 45, 46, 47, 48, 280)[(h >> 16) % 6]
        piped = entry == "fused" and bit(5)
        vpp = dict(method=method, wsize=wsize, direction=bit(0), uniform_color=bit(1), interpolate=bit(2), use_distance_patch=bit(3),
                   use_bilateral_patch=bit(4), c_occ=0.15 if mask != "none" else 0.0, discard_occluded=int(mask == "discard"))
        if vpp["use_distance_patch"]:
            vpp["per_frame_range"] = bit(6)
        if method:
            vpp["wsize_agg_x"] = (64, 9, 1)[i % 3]
        m = None if mask == "none" else ("heur" if entry == "fused" and bit(7) else "given")
        out.append(case(entry, B, 12, W, C=(3, 1)[bit(8)], p=0.06, vpp=vpp, mask=m, D=256 if piped else 64, piped=bool(piped)))
    # behind a D = 256 call of one frame (6592 bytes of LDS): the small variants, whatever the bits above came to
    for W, m in itertools.product((48, 280), (None, "given", "heur")):
        out.append(case("fused", 1, 12, W, p=0.06, vpp=dict(c_occ=0.15) if m else None, mask=m, **PIPE256))
    return out


SWEEP = _sweep_cases()


@gpu
def test_front_route_sweep_is_complete(eng, peng):
    """Both methods, wsize 1..11, no mask / discard / keep, the fused call and VPP alone, and -- spread over the cases -- direction,
    uniform colour, interpolation, distance and bilateral patches, C = 1 / 3, B = 1 / 8 / 33, widths around a multiple of four,
    pipelined or not: every route seen must be a row of the table, every route of the table must be seen here or be in
    ROW_ONLY.  One frame of every case (a different one from case to case) is compared with the oracle; no case is skipped."""
    seen = {}
    for i, c in enumerate(SWEEP):
        got, routes, _ = _run(peng if c["piped"] else eng, c)
        for r in routes:
            assert r in TABLE, f"route {r} reached by case {c} is not covered; add it to the table"
            seen.setdefault(r, c)
        _check(c, got, [i % c["B"]])
    missing = TABLE - set(seen) - set(ROW_ONLY)
    assert not missing, f"table routes the sweep never reached: {sorted(missing)}"
    assert not (set(ROW_ONLY) & set(seen)), f"reached on tiny cases, move out of ROW_ONLY: {sorted(set(ROW_ONLY) & set(seen))}"
    print(f"\n{len(SWEEP)} cases reached {len(seen)} routes: " + ", ".join(sorted(seen)))


# ---- the thresholds: the route flips exactly between the two values, and both sides equal the oracle
def _occ_edge(n, nj):
    return [(case("occ", 1, 40, 52, p=0.1, occ=win(n)), occ(nj))]


EDGES = [
    # W = 2048 | 2049: list entries of 16 | 32 bits (the wide row is cut into parts of at most 1024 columns)
    (case("vpp", 1, 4, 2048, p=0.04), rnd("independent", lb(3))),
    (case("vpp", 1, 4, 2049, p=0.04), rnd("independent", lb(3), rr("u32", seg=3))),
    # B * H = 4095 | 4096: one | four rows per block of the first L pass
    (case("vpp", 1, 4095, 16), rnd("independent", lb(3, 1))),
    (case("vpp", 1, 4096, 16), rnd("independent", lb(3, 4))),
    (case("vpp", 1, 4095, 16, vpp=dict(wsize=7, **MASKED), mask="given"), rnd("inplace", lh(7), rr(modes=(2, 1)))),
    (case("vpp", 1, 4096, 16, vpp=dict(wsize=7, **MASKED), mask="given"), rnd("inplace", lb(7, 4) + ["l_heavy<7>"], rr(modes=(2, 1)))),
    # wsize 7 | 8 | 9: the widest window kernel | the wide kernel (wsize 8 has the radius of 7)
    (case("fused", 2, 24, 64, vpp=dict(wsize=7)), rnd("independent", lb(7))),
    (case("fused", 2, 24, 64, vpp=dict(wsize=8)), rnd("independent", lb(7))),
    (case("fused", 2, 24, 64, vpp=dict(wsize=9)), rnd("independent", ["l_wide"])),
    # window counts: the reachable ones nearest to 64 / 128 / 192 / 256 (WIN holds the (rx, ry) pairs)
    *_occ_edge(64, 1), *_occ_edge(66, 2), *_occ_edge(128, 2), *_occ_edge(130, 3), *_occ_edge(192, 3), *_occ_edge(194, 4),
    *_occ_edge(256, 4), *_occ_edge(258, 0),
    # maxDistance: rad = n + n_agg_y = 15 | 16
    (case("vpp", 1, 40, 64, vpp=dict(method=1, wsize_agg_y=29)), md("wave")),
    (case("vpp", 1, 40, 64, vpp=dict(method=1, wsize_agg_y=31)), md("lds")),
    # 64 W <= 132 KB: W = 2112 | 2113
    (case("vpp", 1, 6, 2112, C=1, p=0.02, vpp=dict(method=1)), md("wave")),
    (case("vpp", 1, 6, 2113, C=1, p=0.02, vpp=dict(method=1)), md("lds")),
    # 2 (2 rad + 1) W <= 60 KB at rad = 16: W = 930 | 931
    (case("vpp", 1, 36, 930, C=1, p=0.02, vpp=dict(method=1, wsize_agg_y=31)), md("lds")),
    (case("vpp", 1, 36, 931, C=1, p=0.02, vpp=dict(method=1, wsize_agg_y=31)), md("global")),
    # the LDS budget behind D = 256 (6592 B = 24 x 274 + 16: that row still fits): 1 | 2 segments at W = 274 | 275, 2 | 3 at 506 | 507
    (case("fused", 2, 8, 274, **PIPE256), rnd("independent", lb(3))),
    (case("fused", 2, 8, 275, **PIPE256), rnd("independent", lb(3), rr(seg=2))),
    (case("fused", 2, 8, 506, **PIPE256), rnd("independent", lb(3), rr(seg=2))),
    (case("fused", 2, 8, 507, **PIPE256), rnd("independent", lb(3), rr(seg=3))),
    # ... and behind D = 192 (36480 B): 1 | 2 at W = 1519 | 1520; not pipelined: one
    (case("fused", 1, 8, 1519, p=0.03, **PIPE192), rnd("independent", lb(3))),
    (case("fused", 1, 8, 1520, p=0.03, **PIPE192), rnd("independent", lb(3), rr(seg=2))),
    (case("fused", 1, 8, 1520, p=0.03, D=192), rnd("independent", lb(3))),
    # 4096 rows behind D = 192 keep four rows per block (36480 >= 18 KB), behind D = 256 they do not (6592 B)
    (case("fused", 2, 2048, 16, **PIPE192), rnd("independent", lb(3, 4))),
    (case("fused", 2, 2048, 16, **PIPE256), rnd("independent", lb(3, 1))),
]


def _edge_id(c):
    kw = ",".join(f"{k}={v}" for k, v in sorted({**c["vpp"], **c["occ"]}.items()))
    return f"{c['entry']}_B{c['B']}_H{c['H']}_W{c['W']}_D{c['D']}{'p' if c['piped'] else ''}_{c['mask']}_{kw}"


@gpu
@pytest.mark.parametrize("c,want", EDGES, ids=[_edge_id(c) for c, _ in EDGES])
def test_front_threshold_edges(eng, peng, c, want):
    got, routes, _ = _run(peng if c["piped"] else eng, c)
    assert sorted(routes) == sorted(want), (c, routes)
    _check(c, got, _frames(c["B"]))


# ---- the trapezoid ring at D = 256 (fused layout: 16 frames of 960 columns): nothing fits next to it, the stand-alone shapes
@gpu
def test_front_routes_behind_the_trapezoid_ring_keep_their_shapes(peng):
    c = case("fused", 16, 32, 960, p=0.03, mask="heur", D=256, piped=True)
    got, routes, back = _run(peng, c)
    assert "sum_trap<16,64,spare>" in back, back
    assert sorted(routes) == sorted(occ(2) + rnd("late", lh(3), rr(modes=(3,)))), routes
    _check(c, got, _frames(c["B"]))


# ---- the list's semantics (include/vppx.h)
@gpu
def test_front_routes_are_reset_per_call_and_leave_last_routes_alone(eng):
    base = case("fused", 2, 24, 64)
    _, first, back = _run(eng, base)
    assert sorted(first) == sorted(rnd("independent", lb(3))) and back and not (set(back) & set(first))
    assert all(not GRAMMAR.match(r) for r in back)
    _, second, back2 = _run(eng, case("vpp", 2, 24, 64, vpp=dict(method=1, direction=0)))
    assert second == md("lds")               # launch order, nothing of the call before
    assert back2 == back                     # a call without rSGM leaves vppx_last_routes as it was
    _, third, back3 = _run(eng, case("occ", 2, 20, 50, p=0.1))
    assert third == occ(2, warp4=False) and back3 == back
    # the same fused call through the helpers of the rSGM table: its list is what it was before this change
    b = _batch(2, 24, 112)
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    lv = torch.empty(b["left"].shape, dtype=torch.uint8, device=eng.device)
    rv = torch.empty_like(lv)
    eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), l_vpp=lv, r_vpp=rv, seed=5, rsgm_kw=dict(dmax=64))
    torch.cuda.synchronize()
    assert eng.last_routes() == ["paths<4,16,exact,census,u8,dirs=ff>", "sum_lr<4,u8,8,64,spare,sw4,fast,16,partw>"]
    lo, ro = _oracle_patterns(b, 1, 5)
    assert np.array_equal(lv[1].cpu().numpy(), lo) and np.array_equal(rv[1].cpu().numpy(), ro)


@gpu
def test_front_routes_of_the_host_wrapper_and_the_drop_ins():
    """pipeline.run_frame queues the heuristic before the fused call proper: one list.  The drop-in scans and
    filter.occlusion_heuristic go through the default context."""
    from vppstereo_amd import _lib, filter as vfilter, pipeline, vpp_core_opt
    fr = synth.make_frame(48, 96, 48, 0.05, seed=5)
    lib, ctx = _lib.load(), _lib.default_context()
    pipeline.run_frame(fr["left"], fr["right"], fr["hints"], maskocc=True, rsgm_kw=dict(dmax=64))
    assert sorted(_lib.last_front_routes(lib, ctx.handle)) == sorted(occ(2) + rnd("late", lh(3), rr(modes=(3,))))
    pipeline.run_frame(fr["left"], fr["right"], fr["hints"], maskocc=False, rsgm_kw=dict(dmax=64))
    assert sorted(_lib.last_front_routes(lib, ctx.handle)) == sorted(rnd("independent", lb(3)))
    want_d, want_c = oracle.occlusion_heuristic(fr["hints"])
    got_d, got_c = vfilter.occlusion_heuristic(fr["hints"])
    assert _lib.last_front_routes(lib, ctx.handle) == occ(2, dmap=True)
    assert np.array_equal(got_d, want_d) and np.array_equal(got_c, want_c)
    l, r, l0, r0 = fr["left"].copy(), fr["right"].copy(), fr["left"].copy(), fr["right"].copy()
    vpp_core_opt.init_rand(3)
    oracle.init_rand(3)
    n = vpp_core_opt.virtual_projection_scan_rnd(l, r, fr["hints"], 96, 48, 3, False, 5, 1, 0.4, 0.1, want_c, False, True)
    n0 = oracle.virtual_projection_scan_rnd(l0, r0, fr["hints"], 96, 48, 3, False, 5, 1, 0.4, 0.1, want_c, False, True)
    assert sorted(_lib.last_front_routes(lib, ctx.handle)) == sorted(rnd("inplace", lh(5), rr(modes=(2, 1))))
    assert n == n0 and np.array_equal(l, l0) and np.array_equal(r, r0)


@gpu
def test_front_routes_of_a_frame_stream_batch():
    """Every batch of a frame stream is one fused call on the stream's context: the list is that batch's."""
    from vppstereo_amd import _lib
    from vppstereo_amd.pipeline import FrameStream
    H, W, D = 24, 64, 64
    frames = [synth.make_frame(H, W, D, 0.06, seed=11, frame=f, channels=1) for f in range(4)]
    rng = np.random.default_rng(4)
    masks = [(rng.random((H, W)) < 0.3).astype(np.uint8) for _ in frames]
    got = []
    with FrameStream(H, W, 1, batch=4, depth=2, seed=SEED, with_g_occ=True, vpp_kw=dict(c_occ=0.15), rsgm_kw=dict(dmax=D),
                     return_patterns=True) as fs:
        for fr, m in zip(frames, masks):
            fs.push(fr["left"][..., 0], fr["right"][..., 0], fr["hints"], m)
        fs.flush()
        for _ in frames:
            got.append(fs.pop())
        assert sorted(_lib.last_front_routes(_lib.load(), fs._ctx.handle)) == sorted(rnd("late", lh(3), rr(modes=(3,))))
    for f, (fr, m) in enumerate(zip(frames, masks)):
        oracle.init_rand(SEED + f)
        lo, ro = oracle.vpp(fr["left"], fr["right"], fr["hints"], g_occ=m, c_occ=0.15)
        assert np.array_equal(got[f][1], lo[..., 0]) and np.array_equal(got[f][2], ro[..., 0]), f


@gpu
def test_front_routes_of_a_graph_replay_are_those_of_the_captured_call():
    import torch
    from vppstereo_amd.engine import Engine
    e = Engine()
    c = case("fused", 2, 24, 64, vpp=MASKED, mask="given")
    inp = _inputs(c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(e.device)
    L, R, Hn, M = t(inp["left"]), t(inp["right"]), t(inp["hints"]), t(inp["mask"])
    out = torch.empty((2, 24, 64), dtype=torch.float32, device=e.device)
    lv = torch.empty((2, 24, 64, 3), dtype=torch.uint8, device=e.device)
    rv = torch.empty_like(lv)
    side = torch.cuda.Stream(device=e.device)
    want = sorted(rnd("late", lh(3), rr(modes=(3,))))
    e.set_graph_mode(True)
    with torch.cuda.stream(side):
        for it in range(4):
            e.vpp_rsgm(L, R, Hn, g_occ=M, out=out, l_vpp=lv, r_vpp=rv, seed=SEED, vpp_kw=dict(MASKED), rsgm_kw=dict(dmax=64))
            side.synchronize()
            assert sorted(e.last_front_routes()) == want, (it, e.last_front_routes())
            if it == 1:   # something else in between: the replay restores the captured call's list
                e.occlusion_heuristic(Hn)
                assert e.last_front_routes() == occ(2)
    assert e.graph_replays() >= 2
    _check(c, dict(l=lv.cpu().numpy(), r=rv.cpu().numpy(), n_hints=None, conf=None, dmap=None), [0, 1])


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, synth
from vppstereo_amd.engine import Engine
b = synth.make_batch(8, 24, 64, 64, 0.05, seed=3)
eng = Engine()
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
lv = torch.empty(b["left"].shape, dtype=torch.uint8, device=eng.device)
rv = torch.empty_like(lv)
eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), l_vpp=lv, r_vpp=rv, seed=5, rsgm_kw=dict(dmax=64))
torch.cuda.synchronize()
print("fused parts", eng.last_call_parts(), "front", ";".join(eng.last_front_routes()), "back", ";".join(eng.last_routes()))
eng.vpp(t(b["left"]), t(b["right"]), t(b["hints"]), seed=5)
torch.cuda.synchronize()
print("alone front", ";".join(eng.last_front_routes()))
np.save(sys.argv[2], lv.cpu().numpy())
"""


@gpu
@pytest.mark.parametrize("env,parts,front", [
    # parts of one context accumulate into its list (5 + 3 frames: the same names, once)
    (dict(VPPX_CHUNK="3"), 2, ";".join(rnd("independent", lb(3)))),
    # the children of VPPX_SUBSTREAMS keep lists of their own, not merged: the call lists nothing, like vppx_last_routes
    (dict(VPPX_SUBSTREAMS="2"), 0, ""),
])
def test_front_routes_of_parts_and_sub_streams(env, parts, front, tmp_path):
    out = str(tmp_path / "lv.npy")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = {ln.split(" ")[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("fused", "alone"))}
    assert lines["fused"].startswith(f"fused parts {parts} front {front} back"), r.stdout
    if "VPPX_SUBSTREAMS" in env:
        assert lines["fused"].endswith("back "), r.stdout
    assert lines["alone"] == "alone front " + ";".join(rnd("independent", lb(3))), r.stdout
    b = synth.make_batch(8, 24, 64, 64, 0.05, seed=3)
    lv = np.load(out)
    for f in (0, 7):
        oracle.init_rand(5 + f)
        lo, _ = oracle.vpp(b["left"][f], b["right"][f], b["hints"][f])
        assert np.array_equal(lv[f], lo), f
