"""CPU: the default rule of the W + sum + WTA route (`wsum<12>`, vppx_wsum_default_route) keeps every case of the route table
of tests/test_gpu_routes.py on the kernels that table pins, and takes the headline's 16-frame parts."""
import ctypes as C
import os

import pytest

from test_gpu_routes import ROUTES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSIMD = 1024   # MI355X: 256 compute units


@pytest.fixture(scope="module")
def rule():
    lib = C.CDLL(os.path.join(ROOT, "vppstereo_amd", "libvppx.so"))
    lib.vppx_wsum_default_route.argtypes = [C.c_int] * 6
    lib.vppx_wsum_default_route.restype = C.c_int
    return lambda B, H, W, D, p2: int(lib.vppx_wsum_default_route(B, -(-H // 16) * 16, -(-W // 16) * 16, D, p2, NSIMD))


@pytest.mark.parametrize("rid,want,c", ROUTES, ids=[r[0] for r in ROUTES])
def test_route_table_rows_keep_their_kernels(rule, rid, want, c):
    assert "wsum<12>" not in want
    assert rule(c["B"], c["H"], c["W"], c["D"], c["p2"]) == 0


def test_the_rule_itself(rule):
    assert rule(16, 540, 960, 192, 35) == 1      # the headline's part: 16 x 544 / 4 = 2176 line quads >= 2 x 1024
    assert rule(16, 540, 960, 192, 61) == 1 and rule(16, 540, 960, 192, 62) == 0   # 3 (24 + P2max) <= 255
    assert rule(15, 540, 960, 192, 35) == 0      # 2040 line quads: below two layers
    assert rule(16, 375, 1242, 192, 35) == 0     # 16 x 384 / 4 = 1536
    assert rule(8, 1536, 2048, 256, 35) == 0 and rule(32, 540, 960, 128, 35) == 0   # D = 192 only
    assert rule(1, 540, 960, 192, 35) == 0
