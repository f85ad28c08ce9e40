"""The convolution kernel at stride 2 (conv_kernels.hip; Engine.raft_conv(..., stride=2), vppx_raft_conv_strided_dt_dev) against the
float64 referee of tests/_strided_ref.py: nn.Conv2d(Cin, Cout, k, stride=2, padding=k // 2) for k 3 and 1.

No atol.  Every finite float32 cell is held to the referee's limit, every bfloat16 cell to the band the single rounding of a
float32 inside that limit can reach.  The output of every case is channels [0, Cout) of a [B, Cout + 2, Ho, Wo] buffer of sentinel
cells with guard cells around it, which must keep the sentinel bit for bit.  What the cases reach, and that the planted mistakes
leave the limit on these very arrays, is asserted on the CPU in tests/test_strided_ref_cpu.py."""
import numpy as np
import pytest

import _conv_ref as CR
import _strided_ref as SR
from _cells import DTYPES, INVALID, SENTINEL16, SENTINEL32, UNSUPPORTED
from _cells import bits as _bits, dev as _dev, guarded as _guarded, guards_intact as _guards_intact, hold, host as _host, tdtype as _tdtype

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EXTRA = 2                                     # channels of the output's buffer behind the Cout the call writes
_REFS = {}


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _ref(name, dtype):
    if (name, dtype) not in _REFS:
        c = SR.case(name, dtype)
        _REFS[name, dtype] = (c, SR.case_ref(c))
    return _REFS[name, dtype]


def _t(eng, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _pack(eng, w, bias, dtype):
    return eng.raft_conv_pack(_t(eng, w), _t(eng, bias), dtype=_tdtype(dtype))


def _route(eng, a, dtype, how):
    """a [B,C,H,W] on the device.  "plain": contiguous; "slice": channels 1 .. C of a [B,C+2,H,W] tensor, frames (C + 2) H W apart."""
    if a is None:
        return None
    if how == "plain":
        return _dev(eng, a, dtype)
    B, Cc, H, W = a.shape
    wide = np.zeros((B, Cc + 2, H, W), F32)
    wide[:, 1:1 + Cc] = a
    return _dev(eng, wide, dtype)[:, 1:1 + Cc]


def _run(eng, c, packed, dtype, how="plain", shift=0, x0=None, x1=None, **kw):
    """The case into channels [0, Cout) of a sentinel-filled [B, Cout + EXTRA, Ho, Wo] inside its guards."""
    import torch
    x0, x1 = c.x0 if x0 is None else x0, c.x1 if x1 is None else x1
    B, Ho, Wo = x0.shape[0], SR.out_size(x0.shape[2]), SR.out_size(x0.shape[3])
    buf, wide = _guarded(eng, (B, c.Cout + EXTRA, Ho, Wo), dtype, shift=shift)
    out = wide[:, :c.Cout]
    got = eng.raft_conv(_route(eng, x0, dtype, how), packed, c.Cout, c.ksize, x1=_route(eng, x1, dtype, how), out=out, stride=2, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.dtype == _tdtype(dtype) and tuple(got.shape) == (B, c.Cout, Ho, Wo)
    raw = _bits(wide[:, c.Cout:])
    assert (raw == (SENTINEL16 if raw.dtype == np.int16 else SENTINEL32)).all(), f"{c.name}: a channel behind the {c.Cout} was written"
    assert _guards_intact(buf, B * (c.Cout + EXTRA) * Ho * Wo, shift=shift), f"{c.name}: a guard cell was written"
    return got


# ---- every case ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SR.CASES))
def test_stride_two_equals_the_referee(eng, name, dtype):
    """3x3: the workgroup tile is 4 rows x 32 columns of OUTPUT pixels; 1x1: 8 x 32.  See the table of tests/_strided_ref.py."""
    c, ref = _ref(name, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    got = _run(eng, c, packed, dtype)
    assert tuple(got.shape[2:]) == (c.Ho, c.Wo) == ((c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1)
    hold(CR, _host(got), ref, f"stride 2 {name}", dtype)
    bits = _bits(got)
    # inputs as channel slices of wider tensors, frame strides above their size: the same bits
    assert np.array_equal(_bits(_run(eng, c, packed, dtype, how="slice")), bits), "slices"
    # an output one cell off its 16 bytes takes the cell route: the same bits
    shifted = _run(eng, c, packed, dtype, shift=1)
    assert shifted.data_ptr() % 16 != 0 and np.array_equal(_bits(shifted), bits), "the cell route"
    if name == "s2_even":
        assert c.Wo % 8 == 0 and got.data_ptr() % 16 == 0 and (got.stride(0) * got.element_size()) % 16 == 0     # the 16-byte route
    # a fresh output: allocated [B,Cout,Ho,Wo], contiguous
    x0, x1 = _dev(eng, c.x0, dtype), None if c.x1 is None else _dev(eng, c.x1, dtype)
    fresh = eng.raft_conv(x0, packed, c.Cout, c.ksize, x1=x1, stride=2)
    assert fresh.is_contiguous() and tuple(fresh.shape) == (c.B, c.Cout, c.Ho, c.Wo) and np.array_equal(_bits(fresh), bits)
    # each frame of the batch equals the one-frame call
    for f in range(c.B):
        one = eng.raft_conv(x0[f:f + 1], packed, c.Cout, c.ksize, x1=None if x1 is None else x1[f:f + 1], stride=2)
        assert np.array_equal(_bits(one), bits[f:f + 1]), f
    if c.B > 1:
        assert not np.array_equal(bits[0], bits[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["s2_even", "d2_even"])
def test_a_width_off_the_group_gives_the_bits_of_the_aligned_route(eng, name, dtype):
    """Two input columns fewer make Wo one less: no multiple of the 16-byte group, so every row goes cell by cell.  No window of the
    output columns that are left reaches the columns taken away, so they must be the aligned run's, bit for bit.  (d2_even's own
    Wo = 33 is off the group: there the narrower map of Wo = 32 is the aligned one.)"""
    c, _ = _ref(name, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    full = _bits(_run(eng, c, packed, dtype))
    cut = _bits(_run(eng, c, packed, dtype, x0=c.x0[:, :, :, :c.W - 2]))
    assert cut.shape[3] == c.Wo - 1 and (c.Wo % 8 == 0) != ((c.Wo - 1) % 8 == 0)
    assert np.array_equal(cut, full[:, :, :, :c.Wo - 1])
    rows = _bits(_run(eng, c, packed, dtype, x0=c.x0[:, :, :c.H - 2]))
    assert np.array_equal(rows, full[:, :, :c.Ho - 1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["enc14", "one1x1", "mask9"])
def test_stride_one_through_the_new_call_is_raft_conv(eng, name, dtype):
    """vppx_raft_conv_strided_dt_dev with stride 1 against Engine.raft_conv (vppx_raft_conv_dt_dev), ReLU and scale included."""
    import torch
    c = CR.case(name, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    x0, x1 = _dev(eng, c.x0, dtype), None if c.x1 is None else _dev(eng, c.x1, dtype)
    want = eng.raft_conv(x0, packed, c.Cout, c.ksize, x1=x1, relu=c.relu, scale=c.scale)
    assert tuple(eng.raft_conv(x0, packed, c.Cout, c.ksize, x1=x1, relu=c.relu, scale=c.scale, stride=1).shape) == tuple(want.shape)
    out = torch.empty_like(want)
    n = c.H * c.W
    eng._bind_stream()
    rc = eng.lib.vppx_raft_conv_strided_dt_dev(x0.data_ptr(), c.C0 * n, c.C0, 0 if x1 is None else x1.data_ptr(), c.C1 * n, c.C1,
                                               packed.data_ptr(), c.Cout, c.ksize, 1, c.B, c.H, c.W, int(c.relu), c.scale, out.data_ptr(),
                                               c.Cout * n, 1 if dtype == "bfloat16" else 0, eng.ctx.handle)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(_bits(out), _bits(want))


def test_one_packed_buffer_serves_either_stride(eng):
    c, ref = _ref("s2_odd", "float32")
    packed = _pack(eng, c.w, c.bias, "float32")
    x0, x1 = _dev(eng, c.x0), _dev(eng, c.x1)
    hold(CR, _host(eng.raft_conv(x0, packed, c.Cout, 3, x1=x1)), SR.case_ref(c, stride=1), "s2_odd at stride 1")
    hold(CR, _host(eng.raft_conv(x0, packed, c.Cout, 3, x1=x1, stride=2, relu=True, scale=.25)), SR.case_ref(c, relu=True, scale=.25),
         "s2_odd at stride 2 with ReLU and scale")
    hold(CR, _host(eng.raft_conv(x0, packed, c.Cout, 3, x1=x1, stride=2)), ref, "s2_odd at stride 2")


# ---- the recording --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_raft_conv_reproduces_the_recorded_block_convolutions(eng, dtype):
    g = SR.load_recording()
    c1_ref, dn_ref = SR.recorded_convs(g, dtype)
    x = g["x"]
    x = _dev(eng, SR.to_bf16(x) if dtype == "bfloat16" else x, dtype)
    c1 = eng.raft_conv(x, _pack(eng, g["conv1.weight"], g["conv1.bias"], dtype), 32, 3, stride=2)
    dn = eng.raft_conv(x, _pack(eng, g["downsample.0.weight"], g["downsample.0.bias"], dtype), 32, 1, stride=2)
    assert tuple(c1.shape) == tuple(dn.shape) == (2, 32, 5, 7)
    hold(CR, _host(c1), c1_ref, "recording: conv1 at stride 2", dtype)
    hold(CR, _host(dn), dn_ref, "recording: downsample[0] at stride 2", dtype)
    if dtype == "float32":                       # the reference's own outputs lie within the same limit of the same value
        assert (np.abs(_host(c1).astype(F64) - g["conv1_out"]) <= 2 * c1_ref.limit).all()
        assert (np.abs(_host(dn).astype(F64) - g["down_out"]) <= 2 * dn_ref.limit).all()


# ---- a NaN cell -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["s2_odd", "d2_odd", "s2_even"])
def test_a_nan_reaches_the_pixels_whose_window_holds_it(eng, name, dtype):
    """3x3: an even-even cell lies in one window, an odd-odd cell in four, an even-odd cell in two, a border cell in what is left of
    those inside the output.  1x1: an even-even cell reaches its pixel, a cell at an odd row or column reaches nothing."""
    c, _ = _ref(name, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    run = lambda x0, x1: eng.raft_conv(_dev(eng, x0, dtype), packed, c.Cout, c.ksize, x1=None if x1 is None else _dev(eng, x1, dtype),   # noqa: E731
                                       relu=True, stride=2)
    base = _bits(run(c.x0, c.x1))
    H, W = c.H, c.W
    cells = [(1, 3, 4, 6), (0, 5, 3, 5), (1, 0, 2, 5), (0, 7, 3, 4), (0, 15, 0, 0), (1, 2, H - 1, W - 1), (0, 9, H - 1, 0), (1, 1, 1, W - 1),
             (0, 4, H - 2, W - 2)]
    counts = set()
    for k, (b, ch, y, x) in enumerate(cells):
        src = "x1" if c.x1 is not None and k % 2 else "x0"
        a = {"x0": c.x0.copy(), "x1": None if c.x1 is None else c.x1.copy()}
        a[src][b, ch, y, x] = np.nan
        got = run(a["x0"], a["x1"])
        nan = np.isnan(_host(got))
        want = np.zeros_like(nan)
        want[b, :] = SR.nan_reach(c.ksize, H, W, y, x)[None]
        counts.add(int(want[b, 0].sum()))
        assert np.array_equal(nan, want), (src, b, ch, y, x)
        assert np.array_equal(_bits(got)[~want], base[~want]), (src, b, ch, y, x)
    assert counts == ({0, 1} if c.ksize == 1 else {1, 2, 4})


# ---- refusals: before anything is launched, with no output byte touched -------------------------------------------------------
def test_refusals_leave_every_byte_alone(eng):
    import torch
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((1 << 16,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((1 << 16,), SENTINEL32, dtype=torch.int32, device=eng.device)
    p, o = inp.data_ptr(), out.data_ptr()
    assert p % 16 == 0
    eng._bind_stream()
    n = 16 * 35                                  # 5 x 7 in, 3 x 4 out

    def conv(x0=p, s0=n, C0=16, x1=p, s1=n, C1=16, packed=p, Cout=14, ksize=3, stride=2, B=2, H=5, W=7, relu=0, scale=1.0, out_=o, so=14 * 12,
             dtype=0):
        return lib.vppx_raft_conv_strided_dt_dev(x0, s0, C0, x1, s1, C1, packed, Cout, ksize, stride, B, H, W, relu, scale, out_, so, dtype, ctx)

    bad = "bad arguments"
    table = (
        # a stride that is not built
        (lambda: conv(stride=0), UNSUPPORTED, "vppx_raft_conv_strided: a stride of 0: 1 and 2 are built"),
        (lambda: conv(stride=3), UNSUPPORTED, "a stride of 3"), (lambda: conv(stride=-2), UNSUPPORTED, "a stride of -2"),
        (lambda: conv(stride=4, ksize=1), UNSUPPORTED, "a stride of 4"),
        # everything vppx_raft_conv_dt_dev refuses, at either stride
        (lambda: conv(x0=None), INVALID, bad), (lambda: conv(x1=None), INVALID, bad), (lambda: conv(packed=None), INVALID, bad),
        (lambda: conv(out_=None), INVALID, bad), (lambda: conv(out_=None, stride=1, so=14 * 35), INVALID, bad),
        (lambda: conv(B=0), INVALID, bad), (lambda: conv(H=0), INVALID, bad), (lambda: conv(W=-1), INVALID, bad),
        (lambda: conv(C0=0), INVALID, "must be positive"), (lambda: conv(C1=-16), INVALID, "C1 not negative"),
        (lambda: conv(Cout=0), INVALID, "must be positive"),
        # a frame stride below its tensor's size: the sources by the input's H x W, out by the output's
        (lambda: conv(s0=n - 1), INVALID, "vppx_raft_conv_strided: x0_frame_stride 559 is less than 16 planes of 5x7"),
        (lambda: conv(s1=0), INVALID, "x1_frame_stride 0"),
        (lambda: conv(so=14 * 12 - 1), INVALID, "out_frame_stride 167 is less than 14 planes of 3x4"),
        (lambda: conv(so=14 * 12, stride=1), INVALID, "out_frame_stride 168 is less than 14 planes of 5x7"),
        (lambda: conv(so=14 * 12 - 1, ksize=1), INVALID, "out_frame_stride 167 is less than 14 planes of 3x4"),
        (lambda: conv(scale=float("nan")), INVALID, "vppx_raft_conv_strided: the scale is not finite"),
        (lambda: conv(dtype=2), INVALID, "vppx_raft_conv_strided: dtype 2"),
        (lambda: conv(packed=p + 8), INVALID, "not 16-byte aligned"),
        (lambda: conv(ksize=2), UNSUPPORTED, "vppx_raft_conv_strided: a kernel size of 2"), (lambda: conv(ksize=7), UNSUPPORTED, "a kernel size of 7"),
        (lambda: conv(C0=8, s0=8 * 35), UNSUPPORTED, "multiples of 16"), (lambda: conv(C1=24, s1=24 * 35), UNSUPPORTED, "multiples of 16"),
        (lambda: conv(C0=512, s0=512 * 35), UNSUPPORTED, "up to 512 in"), (lambda: conv(Cout=257, so=257 * 12), UNSUPPORTED, "1 to 256 out"),
        (lambda: conv(B=1 << 12, H=1 << 10, W=1 << 10, s0=1 << 40, s1=1 << 40, so=1 << 40), UNSUPPORTED, "more than one launch takes"),
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
    for stride in (0, 3, -1):
        with pytest.raises(ValueError, match="stride is"):
            eng.raft_conv(f32(1, 32, 5, 7), packed, 14, 3, stride=stride)
    with pytest.raises(ValueError, match="out: expected shape"):
        eng.raft_conv(f32(1, 32, 5, 7), packed, 14, 3, stride=2, out=f32(1, 14, 5, 7))  # the stride-1 size
    with pytest.raises(ValueError, match="out: expected shape"):
        eng.raft_conv(f32(1, 32, 5, 7), packed, 14, 3, stride=2, out=f32(1, 14, 2, 3))  # the floor
    assert tuple(eng.raft_conv(f32(1, 32, 5, 7), packed, 14, 3, stride=2, out=f32(1, 14, 3, 4)).shape) == (1, 14, 3, 4)
    assert (out.cpu().numpy() == SENTINEL32).all()
