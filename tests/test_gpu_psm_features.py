"""PSMNet's feature_extraction on the library's kernels against the float64 referee of tests/_psm_ref.py: the convolution with
dilation 2 and a residual (Engine.conv2d, vppx_conv2d_dt_dev), the pyramid pooling's average pools (Engine.psm_spp_pool,
vppx_psm_spp_pool_dt_dev) and the assembly into a channel slice (Engine.raft_gru_assemble(out=slice),
vppx_raft_gru_assemble_strided_dt_dev).

No atol.  Every finite float32 cell is held to the referee's limit, every bfloat16 cell to the band the single rounding of a
float32 inside that limit can reach.  A convolution's output is channels [0, Cout) of a [B, Cout + 2, Ho, Wo] buffer of sentinel
cells with guard cells around it, which must keep the sentinel bit for bit.  That the planted mistakes leave the limit on these
very arrays is asserted on the CPU in tests/test_psm_ref_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import _conv_ref as CR
import _gru_ref as G
import _psm_ref as PR
from _cells import DTYPES, INVALID, SENTINEL16, SENTINEL32, UNSUPPORTED
from _cells import bits as _bits, dev as _dev, guarded as _guarded, guards_intact as _guards_intact, hold, host as _host, tdtype as _tdtype

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EXTRA = 2                                     # channels of the output's buffer behind the Cout the call writes


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _t(eng, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _pack(eng, w, bias, dtype):
    return eng.raft_conv_pack(_t(eng, w), _t(eng, bias), dtype=_tdtype(dtype))


def _route(eng, a, dtype, how="plain"):
    """a [B,C,H,W] on the device.  "plain": contiguous; "slice": channels 1 .. C of a [B,C+2,H,W] tensor, frames (C + 2) H W apart."""
    if a is None:
        return None
    if how == "plain":
        return _dev(eng, a, dtype)
    B, Cc, H, W = a.shape
    wide = np.zeros((B, Cc + 2, H, W), F32)
    wide[:, 1:1 + Cc] = a
    return _dev(eng, wide, dtype)[:, 1:1 + Cc]


def _run(eng, c, packed, dtype, res=None, relu=False, scale=1.0, how="plain", shift=0, alias=False, x0=None, x1=None):
    """The case into channels [0, Cout) of a sentinel-filled [B, Cout + EXTRA, H, W] inside its guards.  alias: the residual is
    first copied into those channels and the call reads it from there, out being res itself."""
    import torch
    x0, x1 = c.x0 if x0 is None else x0, c.x1 if x1 is None else x1
    B, H, W = x0.shape[0], x0.shape[2], x0.shape[3]
    buf, wide = _guarded(eng, (B, c.Cout + EXTRA, H, W), dtype, shift=shift)
    out = wide[:, :c.Cout]
    r = None if res is None else _route(eng, res, dtype, how)
    if alias:
        out.copy_(r)
        r = out
    got = eng.conv2d(_route(eng, x0, dtype, how), packed, c.Cout, c.ksize, x1=_route(eng, x1, dtype, how), dilation=c.dilation, residual=r,
                     relu=relu, scale=scale, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.dtype == _tdtype(dtype) and tuple(got.shape) == (B, c.Cout, H, W)
    raw = _bits(wide[:, c.Cout:])
    assert (raw == (SENTINEL16 if raw.dtype == np.int16 else SENTINEL32)).all(), f"a channel behind the {c.Cout} was written"
    assert _guards_intact(buf, B * (c.Cout + EXTRA) * H * W, shift=shift), "a guard cell was written"
    return got


# ---- the dilated convolution: every map with every Cin and Cout under every epilogue ----------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cout", PR.CONV_COUTS)
@pytest.mark.parametrize("cin", PR.CONV_CINS, ids=lambda c: f"{c[0]}+{c[1]}")
@pytest.mark.parametrize("hw", PR.CONV_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dilation_two_equals_the_referee(eng, hw, cin, cout, dtype):
    """Workgroup tile 8 x 32 pixels and 64 channels; a staged image with a two-pixel halo.  Two sources go in as channel slices of
    wider tensors, frame strides above their size."""
    c = PR.make_conv(3, 2, 2, cin[0], cin[1], cout, hw[0], hw[1], dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    how = "slice" if cin[1] else "plain"
    pre = PR.conv2d(c.x0, c.x1, c.w, c.bias, dtype, dilation=2)
    seen = {}
    for res, relu, scale in PR.EPILOGUES:
        ref = PR.conv2d(c.x0, c.x1, c.w, c.bias, dtype, dilation=2, res=c.res if res else None, relu=relu, scale=scale, pre=pre)
        got = _run(eng, c, packed, dtype, c.res if res else None, relu, scale, how=how)
        hold(CR, _host(got), ref, f"dilation 2 {hw} {cin} -> {cout} res={res} relu={relu} scale={scale}", dtype)
        seen[res, relu, scale] = _bits(got)
        if res:                                   # out aliased to res: the same bits
            assert np.array_equal(_bits(_run(eng, c, packed, dtype, c.res, relu, scale, how=how, alias=True)), seen[res, relu, scale])
    # an output one cell off its 16 bytes takes the cell route: the same bits
    shifted = _run(eng, c, packed, dtype, c.res, True, 0.25, how=how, shift=1)
    assert shifted.data_ptr() % 16 != 0 and np.array_equal(_bits(shifted), seen[True, True, 0.25])
    if hw[0] * hw[1] > 4:
        assert not np.array_equal(seen[True, False, 1.0], seen[False, False, 1.0])
    if hw == (8, 32) and not cin[1]:
        got = _run(eng, c, packed, dtype, c.res, True, 0.25)
        assert got.data_ptr() % 16 == 0 and (got.stride(0) * got.element_size()) % 16 == 0                     # the 16-byte route


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["d1_res", "k1_d2"])
def test_dilation_one_with_a_residual_and_the_1x1_at_dilation_two(eng, name, dtype):
    c = PR.conv_case(name, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    got = _run(eng, c, packed, dtype, c.res, c.relu, c.scale, how="slice")
    hold(CR, _host(got), PR.conv_case_ref(c), name, dtype)
    assert np.array_equal(_bits(_run(eng, c, packed, dtype, c.res, c.relu, c.scale, alias=True)), _bits(got))
    if name == "k1_d2":                           # the 1x1 itself: the bits of dilation 1
        c.dilation = 1
        assert np.array_equal(_bits(_run(eng, c, packed, dtype, c.res, c.relu, c.scale)), _bits(got))


def test_a_13_wide_map_goes_cell_by_cell_with_the_bits_of_the_padded_one(eng):
    """float32, W = 13: no row is a whole number of 16-byte groups.  The same data with three columns of +0 behind every row (the
    +0 the staging writes outside a map) on the 16-byte route: the same sums in the same order."""
    c = PR.make_conv(3, 2, 2, 16, 0, 20, 9, 13)
    packed = _pack(eng, c.w, c.bias, "float32")
    pad = lambda a: np.pad(a, ((0, 0), (0, 0), (0, 0), (0, 3)))                                                # noqa: E731
    narrow = _bits(_run(eng, c, packed, "float32", c.res, True, 0.25))
    wide = _bits(_run(eng, c, packed, "float32", pad(c.res), True, 0.25, x0=pad(c.x0)))
    assert wide.shape[3] == 16 and np.array_equal(narrow, wide[:, :, :, :13])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_reaches_the_nine_pixels_two_apart(eng, dtype):
    c = PR.make_conv(3, 2, 2, 16, 32, 20, 9, 33, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    run = lambda x0, x1: eng.conv2d(_dev(eng, x0, dtype), packed, c.Cout, 3, x1=_dev(eng, x1, dtype), dilation=2, relu=True)    # noqa: E731
    base = _bits(run(c.x0, c.x1))
    H, W = c.H, c.W
    counts = set()
    for k, (b, ch, y, x) in enumerate([(1, 3, 4, 6), (0, 5, 3, 31), (0, 15, 0, 0), (1, 2, H - 1, W - 1), (0, 9, H - 1, 0), (1, 1, 1, W - 2)]):
        src = "x1" if k % 2 else "x0"
        a = {"x0": c.x0.copy(), "x1": c.x1.copy()}
        a[src][b, ch, y, x] = np.nan
        got = run(a["x0"], a["x1"])
        nan = np.isnan(_host(got))
        want = np.zeros_like(nan)
        want[b, :] = PR.nan_reach(H, W, y, x)[None]
        counts.add(int(want[b, 0].sum()))
        assert np.array_equal(nan, want), (src, b, ch, y, x)
        assert np.array_equal(_bits(got)[~want], base[~want]), (src, b, ch, y, x)
    assert counts == {4, 6, 9}                    # a corner, an edge, the interior


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("name", ["enc14", "one1x1"])
def test_dilation_one_without_a_residual_is_the_strided_call(eng, name, stride, dtype):
    c = CR.case(name, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    x0, x1 = _dev(eng, c.x0, dtype), None if c.x1 is None else _dev(eng, c.x1, dtype)
    want = eng.raft_conv(x0, packed, c.Cout, c.ksize, x1=x1, relu=c.relu, scale=c.scale, stride=stride)
    got = eng.conv2d(x0, packed, c.Cout, c.ksize, x1=x1, stride=stride, relu=c.relu, scale=c.scale)
    assert tuple(got.shape) == tuple(want.shape) and np.array_equal(_bits(got), _bits(want))


def test_conv2d_refusals_leave_every_byte_alone(eng):
    import torch
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((1 << 16,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((1 << 16,), SENTINEL32, dtype=torch.int32, device=eng.device)
    p, o = inp.data_ptr(), out.data_ptr()
    eng._bind_stream()
    n = 16 * 35

    def conv(x0=p, s0=n, C0=16, x1=p, s1=n, C1=16, packed=p, Cout=14, ksize=3, stride=1, dilation=2, B=2, H=5, W=7, res=p, sr=14 * 35, relu=0,
             scale=1.0, out_=o, so=14 * 35, dtype=0):
        return lib.vppx_conv2d_dt_dev(x0, s0, C0, x1, s1, C1, packed, Cout, ksize, stride, dilation, B, H, W, res, sr, relu, scale, out_, so,
                                      dtype, ctx)

    bad = "bad arguments"
    table = (
        (lambda: conv(dilation=0), UNSUPPORTED, "vppx_conv2d: a dilation of 0 at stride 1"), (lambda: conv(dilation=3), UNSUPPORTED, "a dilation of 3"),
        (lambda: conv(dilation=-2), UNSUPPORTED, "a dilation of -2"),
        (lambda: conv(stride=2, so=14 * 12, sr=14 * 12), UNSUPPORTED, "a dilation of 2 at stride 2"),
        (lambda: conv(stride=2, ksize=1, so=14 * 12, sr=14 * 12), UNSUPPORTED, "a dilation of 2 at stride 2"),
        # the checker's order: the stride in front of the dilation, the dilation in front of the channels and the frame strides
        (lambda: conv(stride=3, dilation=3), UNSUPPORTED, "a stride of 3"), (lambda: conv(dilation=3, C0=8), UNSUPPORTED, "a dilation of 3"),
        (lambda: conv(dilation=3, sr=1), UNSUPPORTED, "a dilation of 3"), (lambda: conv(scale=float("inf"), dilation=3), INVALID, "not finite"),
        # the residual's frame stride, by the output's size, in front of out's
        (lambda: conv(sr=14 * 35 - 1), INVALID, "vppx_conv2d: res_frame_stride 489 is less than 14 planes of 5x7"),
        (lambda: conv(sr=14 * 35 - 1, so=1), INVALID, "res_frame_stride 489"), (lambda: conv(sr=0), INVALID, "res_frame_stride 0"),
        (lambda: conv(dilation=1, stride=2, sr=14 * 12 - 1, so=14 * 12), INVALID, "res_frame_stride 167 is less than 14 planes of 3x4"),
        (lambda: conv(s0=n - 1, sr=1), INVALID, "x0_frame_stride 559"),
        # everything the strided call refuses
        (lambda: conv(x0=None), INVALID, bad), (lambda: conv(x1=None), INVALID, bad), (lambda: conv(packed=None), INVALID, bad),
        (lambda: conv(out_=None), INVALID, bad), (lambda: conv(B=0), INVALID, bad), (lambda: conv(H=0), INVALID, bad), (lambda: conv(W=-1), INVALID, bad),
        (lambda: conv(C0=0), INVALID, "must be positive"), (lambda: conv(C1=-16), INVALID, "C1 not negative"), (lambda: conv(Cout=0), INVALID, "must be positive"),
        (lambda: conv(s1=0), INVALID, "x1_frame_stride 0"), (lambda: conv(so=14 * 35 - 1), INVALID, "out_frame_stride 489 is less than 14 planes of 5x7"),
        (lambda: conv(scale=float("nan")), INVALID, "vppx_conv2d: the scale is not finite"), (lambda: conv(dtype=2), INVALID, "vppx_conv2d: dtype 2"),
        (lambda: conv(packed=p + 8), INVALID, "not 16-byte aligned"), (lambda: conv(ksize=2), UNSUPPORTED, "a kernel size of 2"),
        (lambda: conv(stride=0), UNSUPPORTED, "a stride of 0"), (lambda: conv(C0=8, s0=8 * 35), UNSUPPORTED, "multiples of 16"),
        (lambda: conv(C0=512, s0=512 * 35), UNSUPPORTED, "up to 512 in"), (lambda: conv(Cout=257, so=257 * 35, sr=257 * 35), UNSUPPORTED, "1 to 256 out"),
    )
    for k, (call, code, msg) in enumerate(table):
        rc = call()
        text = lib.vppx_last_error().decode()
        assert rc == code and msg in text, (k, rc, code, msg, text)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL32).all() and (inp.cpu().numpy() == 1.0).all()
    # through Engine
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=eng.device)            # noqa: E731
    packed = eng.raft_conv_pack(f32(14, 32, 3, 3))
    for kw in (dict(dilation=3), dict(dilation=0), dict(dilation=2, stride=2)):
        with pytest.raises(ValueError, match="dilation is"):
            eng.conv2d(f32(1, 32, 5, 7), packed, 14, 3, **kw)
    with pytest.raises(ValueError, match="residual: expected shape"):
        eng.conv2d(f32(1, 32, 5, 7), packed, 14, 3, dilation=2, residual=f32(1, 14, 3, 4))
    with pytest.raises(ValueError, match="residual: expected"):
        eng.conv2d(f32(1, 32, 5, 7), packed, 14, 3, dilation=2, residual=f32(1, 14, 5, 7).bfloat16())
    assert (out.cpu().numpy() == SENTINEL32).all()


# ---- the pools --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(PR.POOL_CASES))
def test_the_pools_equal_the_referee(eng, name, dtype):
    """x as channels 1 .. C of a [B,C+2,H,W] tensor: a frame stride above the frame."""
    c = PR.pool_case(name, dtype)
    x = _route(eng, c.x, dtype, "slice")
    assert c.B == 1 or x.stride(0) > c.C * c.H * c.W
    outs = eng.psm_spp_pool(x, c.ks)
    again = eng.psm_spp_pool(_dev(eng, c.x, dtype), c.ks)
    assert len(outs) == len(c.ks)
    for k, got, same in zip(c.ks, outs, again):
        assert got.is_contiguous() and got.dtype == _tdtype(dtype) and tuple(got.shape) == (c.B, c.C, c.H // k, c.W // k)
        hold(PR, _host(got), PR.pool(c.x, k), f"pool {name} k={k}", dtype)
        assert np.array_equal(_bits(got), _bits(same)), "the contiguous input"
        one = eng.psm_spp_pool(x, (k,))[0]         # a level alone: another grid, another order, the same limit
        hold(PR, _host(one), PR.pool(c.x, k), f"pool {name} k={k} alone", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["odd", "spp", "direct"])
def test_a_nan_behind_the_floor_boundary_reaches_nothing_of_its_level(eng, name, dtype):
    c = PR.pool_case(name, dtype)
    base = [_bits(t) for t in eng.psm_spp_pool(_dev(eng, c.x, dtype), c.ks)]
    for (y, x) in ((c.H - 1, 3), (5, c.W - 1), (c.H - 1, c.W - 1), (0, 0), (c.H // 2, c.W // 2)):
        a = c.x.copy()
        a[c.B - 1, 1, y, x] = np.nan
        for k, got, was in zip(c.ks, eng.psm_spp_pool(_dev(eng, a, dtype), c.ks), base):
            nan = np.isnan(_host(got))
            want = np.zeros_like(nan)
            if y < (c.H // k) * k and x < (c.W // k) * k:
                want[c.B - 1, 1, y // k, x // k] = True
            assert np.array_equal(nan, want), (k, y, x)
            assert np.array_equal(_bits(got)[~want], was[~want]), (k, y, x)


def test_pool_refusals_leave_every_byte_alone(eng):
    import torch
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((1 << 16,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((1 << 16,), SENTINEL32, dtype=torch.int32, device=eng.device)
    p, o = inp.data_ptr(), out.data_ptr()
    eng._bind_stream()

    def pool(x=p, sx=3 * 70 * 72, B=2, Cc=3, H=70, W=72, n=2, ks=(8, 64), outs=(o, o + 4096), dtype=0, no_ks=False, no_outs=False):
        ka = None if no_ks else (C.c_int * 4)(*ks)
        oa = None if no_outs else (C.c_void_p * 4)(*outs)
        return lib.vppx_psm_spp_pool_dt_dev(x, sx, B, Cc, H, W, n, ka, oa, dtype, ctx)

    table = (
        (lambda: pool(x=None), INVALID, "vppx_psm_spp_pool: bad arguments"), (lambda: pool(no_ks=True), INVALID, "bad arguments"),
        (lambda: pool(no_outs=True), INVALID, "bad arguments"), (lambda: pool(outs=(o, None)), INVALID, "level 1: bad arguments"),
        (lambda: pool(B=0), INVALID, "must be positive"), (lambda: pool(Cc=0), INVALID, "must be positive"), (lambda: pool(H=-1), INVALID, "must be positive"),
        (lambda: pool(W=0), INVALID, "must be positive"), (lambda: pool(n=0), INVALID, "0 levels, 1 .. 4"), (lambda: pool(n=5), INVALID, "5 levels"),
        (lambda: pool(ks=(8, 0)), INVALID, "level 1: a window of 0"), (lambda: pool(ks=(-1, 8)), INVALID, "level 0: a window of -1"),
        (lambda: pool(H=63), INVALID, "level 1: a window of 64 over a 63x72 map leaves no cell"), (lambda: pool(W=7, sx=3 * 70 * 7), INVALID, "level 0"),
        (lambda: pool(sx=3 * 70 * 72 - 1), INVALID, "x_frame_stride 15119 is less than 3 planes of 70x72"), (lambda: pool(dtype=2), INVALID, "dtype 2"),
        (lambda: pool(ks=(8, 65)), UNSUPPORTED, "level 1: a window of 65, up to 64 are built"), (lambda: pool(ks=(128, 8)), UNSUPPORTED, "a window of 128"),
    )
    for k, (call, code, msg) in enumerate(table):
        rc = call()
        text = lib.vppx_last_error().decode()
        assert rc == code and msg in text, (k, rc, code, msg, text)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL32).all() and (inp.cpu().numpy() == 1.0).all()
    x = torch.zeros((1, 3, 70, 72), dtype=torch.float32, device=eng.device)
    for ks in ((), (1, 2, 3, 4, 5), (0,), (65,), (71,)):
        with pytest.raises(ValueError, match="ks:"):
            eng.psm_spp_pool(x, ks)
    with pytest.raises(TypeError):
        eng.psm_spp_pool(x.double())


# ---- the assembly into a channel slice --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(8, 9), (12, 16)], ids=["8x9", "12x16"])
def test_assemble_into_a_channel_slice(eng, hw, dtype):
    """Four interp sources of 1x1, 2x3, 4x4 and 8x9 cells into channels 5 .. of a wider tensor: the contiguous call's bits, the
    referee's values, and a sentinel in every cell outside the slice.  12 x 16 puts the slice on the 16-byte route."""
    import torch
    H, W = hw
    rng = np.random.default_rng([7303, H, W])
    B, sizes, chans = 2, ((1, 1), (2, 3), (4, 4), (8, 9)), (3, 2, 4, 3)
    import _gruconv_ref as R
    arrs = [R._cells(rng, (B, ch) + s, dtype) for ch, s in zip(chans, sizes)]
    srcs = [(_dev(eng, a, dtype), "interp") for a in arrs]
    total = sum(chans)
    flat = torch.empty((B, total, H, W), dtype=_tdtype(dtype), device=eng.device)
    eng.raft_gru_assemble(srcs, out=flat)
    hold(G, _host(flat), G.assemble([(a, "interp") for a in arrs], H, W), f"assemble {hw}", dtype)
    buf, wide = _guarded(eng, (B, total + 9, H, W), dtype)
    out = wide[:, 5:5 + total]
    got = eng.raft_gru_assemble(srcs, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and not out.is_contiguous()
    assert np.array_equal(_bits(got), _bits(flat))
    sent = SENTINEL16 if dtype == "bfloat16" else SENTINEL32
    assert (_bits(wide[:, :5]) == sent).all() and (_bits(wide[:, 5 + total:]) == sent).all() and _guards_intact(buf, B * (total + 9) * H * W)
    # the strided entry point with the contiguous tensor's stride: the bits of the contiguous call
    from vppstereo_amd import _lib
    arr = (_lib.VppxGruSource * 4)(*[_lib.VppxGruSource(t.data_ptr(), t.shape[1] * t.shape[2] * t.shape[3], t.shape[1], t.shape[2], t.shape[3],
                                                         _lib.GRU_MODES["interp"]) for t, _ in srcs])
    again = torch.empty_like(flat)
    dt = 1 if dtype == "bfloat16" else 0
    eng._bind_stream()
    assert eng.lib.vppx_raft_gru_assemble_strided_dt_dev(arr, 4, B, H, W, again.data_ptr(), total * H * W, dt, eng.ctx.handle) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(again), _bits(flat))
    canary = _bits(again).copy()
    assert eng.lib.vppx_raft_gru_assemble_strided_dt_dev(arr, 4, B, H, W, again.data_ptr(), total * H * W - 1, dt, eng.ctx.handle) == INVALID
    assert "out_frame_stride" in eng.lib.vppx_last_error().decode()
    assert eng.lib.vppx_raft_gru_assemble_strided_dt_dev(arr, 4, B, H, W, None, total * H * W, dt, eng.ctx.handle) == INVALID
    assert eng.lib.vppx_raft_gru_assemble_strided_dt_dev(arr, 5, B, H, W, again.data_ptr(), total * H * W, dt, eng.ctx.handle) == INVALID
    torch.cuda.synchronize()
    assert np.array_equal(_bits(again), canary)
    with pytest.raises(ValueError, match="out: expected"):
        eng.raft_gru_assemble(srcs, out=wide[:, 5:5 + total - 1])


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------
def _wrapper_engine():
    """The Engine FusedFeatureExtraction launches on."""
    import torch
    from vppstereo_amd.corr import _engine
    return _engine(torch.device("cuda", torch.cuda.current_device()))


def _load(module, g, prefix):
    import torch
    module.load_state_dict({k[len(prefix):]: torch.from_numpy(np.asarray(g[k])) for k in g.files
                            if k.startswith(prefix) and k[len(prefix):] in module.state_dict()})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(PR.RECORDED_BLOCKS))
def test_the_wrapper_runs_the_recorded_blocks(name, dtype):
    """The reference's own BasicBlock(16, 16, 1, None, 1, 2) and BasicBlock(16, 32, 2, downsample, 1, 1): 2 and 3 launches."""
    import torch
    import _raft_loop as L
    from vppstereo_amd.psmnet import FusedFeatureExtraction
    g = PR.load_recording()
    fe = PR.standin(widths=(16, 32, 16, 16), blocks=(1, 1, 1, 1))
    blk = fe.layer4[0] if name == "a" else fe.layer2[0]
    _load(blk, g, name + ".")
    eng = _wrapper_engine()
    wrapped = FusedFeatureExtraction(fe.to(eng.device))
    x = g[f"{name}.x"]
    x = PR.to_bf16(x) if dtype == "bfloat16" else x
    with torch.no_grad(), L.LaunchSpy(eng, ("conv2d",)) as spy:
        got = wrapped._block(eng, blk, _dev(eng, x, dtype))
    assert len(spy.records) == (2 if name == "a" else 3) and got.dtype == _tdtype(dtype)
    ref = PR.block(x, g, name, dtype, **PR.RECORDED_BLOCKS[name])
    hold(CR, _host(got), ref, f"recorded block {name}", dtype)
    if name == "b":                               # the downsample's launch runs first, and its output is the residual
        assert spy.records[0].args[3] == 1 and np.array_equal(L._np(spy.records[2].kwargs["residual"]), L._np(spy.records[0].result))
        hold(CR, L._np(spy.records[0].result), ref.down, "recorded block b: downsample", dtype)
    hold(CR, L._np(spy.records[-2].result), ref.hidden, f"recorded block {name}: conv1", dtype)
    if dtype == "float32":                        # the reference's own output lies within the same limit of the same value
        assert (np.abs(_host(got).astype(F64) - g[f"{name}.out"]) <= 2 * ref.limit).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_wrapper_runs_the_recorded_tail(dtype):
    """Pool, branch convolutions and the strided assemble on the recorder's 64 x 72 map: the sampled rows and the channel order."""
    import torch
    from vppstereo_amd.psmnet import FusedFeatureExtraction
    g = PR.load_recording()
    fe = PR.standin(widths=(16, 64, 16, 128), blocks=(1, 1, 1, 1), branch=32)
    for k in (1, 2, 3, 4):
        _load(getattr(fe, f"branch{k}"), g, f"tail.branch{k}.")
    eng = _wrapper_engine()
    wrapped = FusedFeatureExtraction(fe.to(eng.device))
    raw, skip = PR.tail_raw_skip()
    if dtype == "bfloat16":
        raw, skip = PR.to_bf16(raw), PR.to_bf16(skip)
    buf = torch.full((1, 320, 64, 72), float("nan"), dtype=_tdtype(dtype), device=eng.device)
    buf[:, :64], buf[:, 64:192] = _dev(eng, raw, dtype), _dev(eng, skip, dtype)
    with torch.no_grad():
        out = wrapped._tail(eng, buf)
    assert out.data_ptr() == buf.data_ptr()
    ref = PR.tail(raw, skip, PR.recorded_branches(g), dtype)
    got = _host(out)
    hold(CR, got, ref, "recorded tail", dtype)
    assert np.array_equal(got[:, :64], raw) and np.array_equal(got[:, 64:192], skip)          # neither copied nor touched
    if dtype == "float32":
        rows, heads = list(g["tail.rows"]), list(g["tail.heads"])
        assert np.array_equal(got[:, heads][:, :, rows], g["tail.heads_out"])
        lim = ref.limit[:, 192:][:, :, rows]
        assert (np.abs(got[:, 192:][:, :, rows].astype(F64) - g["tail.branches_out"]) <= 2 * lim).all()
        wrong = PR.tail(raw, skip, PR.recorded_branches(g), planted="order_1234").value[:, 192:][:, :, rows]
        assert (np.abs(got[:, 192:][:, :, rows] - wrong) > 2 * lim).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_launch_of_the_wrapper_is_held_to_its_referee(dtype, monkeypatch):
    """A stand-in of the reference's structure, widths 16 / 16 / 32 / 32 and two blocks in layer2, on a [2,3,256,288] input: only
    the stem runs in torch, nothing is concatenated, and the launches are the documented 22."""
    import torch
    import _raft_loop as L
    from vppstereo_amd.psmnet import FusedFeatureExtraction
    eng = _wrapper_engine()
    fe = PR.standin().to(eng.device)
    wrapped = FusedFeatureExtraction(fe, dtype=_tdtype(dtype))
    x = torch.rand((2, 3, 256, 288), generator=torch.Generator().manual_seed(7502)).to(eng.device) * 2 - 1
    ran = []
    hooks = [m.register_forward_hook(lambda mod, i, o, n=n: ran.append(n)) for n, m in fe.named_modules()
             if isinstance(m, (torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.AvgPool2d))]

    def no_cat(*a, **k):
        raise AssertionError("torch.cat ran")

    monkeypatch.setattr(torch, "cat", no_cat)
    monkeypatch.setattr(torch.nn.functional, "interpolate", no_cat)
    with L.LaunchSpy(eng, ("conv2d", "psm_spp_pool", "raft_gru_assemble")) as spy:
        out = wrapped(x)
    torch.cuda.synchronize()
    monkeypatch.undo()
    for h in hooks:
        h.remove()
    assert ran == ["firstconv.0.0", "firstconv.0.1"], ran
    assert tuple(out.shape) == (2, 16, 64, 72) and out.dtype == _tdtype(dtype) and bool(torch.isfinite(out.float()).all())
    assert len(spy.records) == wrapped.launches() == 22
    assert [r.name for r in spy.records] == ["conv2d"] * 14 + ["psm_spp_pool"] + ["conv2d"] * 4 + ["raft_gru_assemble"] + ["conv2d"] * 2
    plan = PR.launch_plan(fe)
    convs = spy.of("conv2d")
    assert len(plan) == len(convs) == 20
    for k, (rec, (conv, bn, relu)) in enumerate(zip(convs, plan)):
        PR.check_conv_launch(rec, conv, bn, relu, f"launch {k}")
    # blocks: the residual of a second convolution is the downsample's output, or the block's input
    assert np.array_equal(L._np(convs[3].kwargs["residual"]), L._np(convs[2].args[0]))          # layer1[0]: x itself
    assert np.array_equal(L._np(convs[6].kwargs["residual"]), L._np(convs[4].result))           # layer2[0]: downsample first
    pool = spy.of("psm_spp_pool")[0]
    skip = L._np(pool.args[0])
    assert tuple(pool.args[1]) == (8, 16, 32, 64) and skip.shape == (2, 32, 64, 72)
    assert np.array_equal(skip, L._np(convs[13].result))                                         # output_skip, read in place
    for k, got in zip(pool.args[1], pool.result):
        hold(PR, L._np(got), PR.pool(skip, k), f"the wrapper's pool k={k}", dtype)
    asm = spy.of("raft_gru_assemble")[0]
    srcs = [(L._np(t), mode) for t, mode in asm.args[0]]
    assert [m for _, m in srcs] == ["interp"] * 4 and [s.shape[2:] for s, _ in srcs] == [(8, 9), (4, 4), (2, 2), (1, 1)]
    hold(G, L._np(asm.out["out"]), G.assemble(srcs, 64, 72), "the wrapper's assemble", dtype)
    # lastconv reads the one buffer: output_raw, output_skip and the four branches, in the reference's order
    feat = L._np(convs[18].args[0])
    assert feat.shape == (2, 16 + 32 + 64, 64, 72)
    assert np.array_equal(feat[:, :16], L._np(convs[7 + 1].result)) and np.array_equal(feat[:, 16:48], skip)
    assert np.array_equal(feat[:, 48:], L._np(asm.out["out"]))
