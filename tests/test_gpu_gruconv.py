"""The 3x3 convolution on the matrix cores and the ConvGRU made of it (conv_kernels.hip; Engine.raft_conv3x3, raft_gru_zr,
raft_gru_q; vppstereo_amd.update with conv=True) against the float64 referee of tests/_gruconv_ref.py.

No atol.  Every finite float32 cell is held to the referee's limit, every bfloat16 cell to the band the single rounding of a
float32 inside that limit can reach; a cell that is not finite must have the referee's class.  Sentinel cells in front of and
behind every output must be intact.  What the cases reach, and that the planted mistakes leave the limit on these very arrays,
is asserted on the CPU in tests/test_gruconv_ref_cpu.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import _gru_ref as G
import _gruconv_ref as R
from _cells import DTYPES, INVALID, SENTINEL32, UNSUPPORTED
from _cells import bits as _bits, dev as _dev, guarded as _guarded, guards_intact as _guards_intact, hold, host as _host, tdtype as _tdtype

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
_REFS = {}


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _conv_ref(name, dtype):
    if (name, dtype) not in _REFS:
        c = R.case(name, dtype)
        _REFS[name, dtype] = (c, R.case_ref(c))
    return _REFS[name, dtype]


def _gru_ref(name, dtype):
    if ("gru", name, dtype) not in _REFS:
        c = R.gru_case(name, dtype)
        _REFS["gru", name, dtype] = (c, R.gru_case_ref(c))
    return _REFS["gru", name, dtype]


def _route(eng, a, dtype, how):
    """a [B,C,H,W] on the device.  how = "plain": contiguous; "slice": channels 1 .. C of a [B,C+2,H,W] tensor; "shift": a
    contiguous tensor one cell into its buffer."""
    import torch
    if a is None:
        return None
    B, Cc, H, W = a.shape
    if how == "plain":
        return _dev(eng, a, dtype)
    if how == "slice":
        wide = np.zeros((B, Cc + 2, H, W), F32)
        wide[:, 1:1 + Cc] = a
        return _dev(eng, wide, dtype)[:, 1:1 + Cc]
    flat = torch.zeros((a.size + 1,), dtype=_tdtype(dtype), device=eng.device)
    t = flat[1:].view(*a.shape)
    t.copy_(_dev(eng, a, dtype))
    assert t.data_ptr() % 16 != 0
    return t


def _pack(eng, w, bias, dtype):
    import torch
    return eng.raft_conv3x3_pack(torch.from_numpy(w).to(eng.device), None if bias is None else torch.from_numpy(bias).to(eng.device),
                                 dtype=_tdtype(dtype))


# ---- the plain epilogue --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_conv_equals_the_referee(eng, name, dtype):
    """The kernel's workgroup tile is 8 rows x 32 columns of one frame x 64 output channels, and K runs in chunks of 32
    (bfloat16) or 16 (float32) input channels.  "tiles" (2 frames of 40x72, 32 channels in) crosses it more than twice in
    every direction the kernel tiles: five tiles of rows, three of columns of which the last is 8 wide, two frames (the
    frame is the slowest index of the grid), and one (bfloat16) or two (float32) chunks; "deep_zr" crosses the 64 output
    channels four times and K twelve (bfloat16) or twenty-four (float32) times."""
    import torch
    c, ref = _conv_ref(name, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    assert packed.dtype == torch.uint8 and packed.numel() == eng.lib.vppx_raft_conv3x3_packed_bytes(c.Cout, c.C0 + c.C1, 1 if dtype == "bfloat16" else 0)
    shape = (c.B, c.Cout, c.H, c.W)
    buf, out = _guarded(eng, shape, dtype)
    x0, x1 = _route(eng, c.x0, dtype, "plain"), _route(eng, c.x1, dtype, "plain")
    got = eng.raft_conv3x3(x0, packed, c.Cout, x1=x1, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.dtype == _tdtype(dtype)
    hold(R, _host(got), ref, f"conv {name}", dtype)
    assert _guards_intact(buf, int(np.prod(shape)))
    bits = _bits(got)
    # with the ReLU: monotone and 1-Lipschitz, the same limit around relu(value)
    relu = eng.raft_conv3x3(x0, packed, c.Cout, x1=x1, relu=True)
    hold(R, _host(relu), R._ns(R._relu(ref.value), ref.limit), f"conv {name} relu", dtype)
    assert (_host(relu) >= 0).all() and relu.shape == shape
    # a fresh output: the same bits
    assert np.array_equal(_bits(eng.raft_conv3x3(x0, packed, c.Cout, x1=x1)), bits)
    if not name.startswith("deep"):
        nob = eng.raft_conv3x3(x0, _pack(eng, c.w, None, dtype), c.Cout, x1=x1)
        hold(R, _host(nob), R.case_ref(c, use_bias=False), f"conv {name} without a bias", dtype)
    if name == "odd":
        # the same data through channel slices of wider tensors, and through tensors and an output one cell off their buffers'
        # boundaries, which takes the cell-by-cell route: the same bits
        for how, shift in (("slice", 0), ("shift", 1)):
            buf2, out2 = _guarded(eng, shape, dtype, shift=shift)
            eng.raft_conv3x3(_route(eng, c.x0, dtype, how), packed, c.Cout, x1=_route(eng, c.x1, dtype, how), out=out2)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(out2), bits), how
            assert _guards_intact(buf2, int(np.prod(shape)), shift=shift)
    if c.B > 1:                          # each frame of a batch equals the one-frame call
        assert not np.array_equal(bits[0], bits[1])
        for f in range(c.B):
            one = eng.raft_conv3x3(x0[f:f + 1], packed, c.Cout, x1=None if x1 is None else x1[f:f + 1])
            assert np.array_equal(_bits(one), bits[f:f + 1]), f


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_reaches_its_3x3_pixels_and_nothing_else(eng, dtype):
    c, _ = _conv_ref("odd", dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    base = _bits(eng.raft_conv3x3(_dev(eng, c.x0, dtype), packed, c.Cout, x1=_dev(eng, c.x1, dtype)))
    for src, (b, ch, y, x) in (("x1", (1, 3, 7, 20)), ("x0", (0, 15, 0, 0)), ("x0", (2, 0, c.H - 1, c.W - 1)), ("x1", (0, 9, 8, 31))):
        a = {"x0": c.x0.copy(), "x1": c.x1.copy()}
        a[src][b, ch, y, x] = np.nan
        got = eng.raft_conv3x3(_dev(eng, a["x0"], dtype), packed, c.Cout, x1=_dev(eng, a["x1"], dtype))
        nan = np.isnan(_host(got))
        want = np.zeros_like(nan)
        want[b, :, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
        assert np.array_equal(nan, want), (src, b, ch, y, x)
        assert np.array_equal(_bits(got)[~want], base[~want]), (src, b, ch, y, x)


# ---- the gates -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(R.GRU_CASES))
def test_zr_and_q_equal_the_referee(eng, name, dtype):
    import torch
    c, ref = _gru_ref(name, dtype)
    Cc, W = c.C, c.weights
    packed_zr = _pack(eng, np.concatenate([W["convz_weight"], W["convr_weight"]]), np.concatenate([W["convz_bias"], W["convr_bias"]]), dtype)
    packed_q = _pack(eng, W["convq_weight"], W["convq_bias"], dtype)
    shape = (c.B, Cc, c.H, c.W)
    n = int(np.prod(shape))

    def run(how, shift):
        d = lambda a: _route(eng, a, dtype, how)                                           # noqa: E731
        hx = d(np.concatenate([c.h, c.x], axis=1))
        h = d(c.h)
        cz, cr, cq = _dev(eng, c.ctx, dtype).split(Cc, dim=1)       # views of one [B,3C,H,W] tensor: frames 3C*H*W apart
        if how == "shift":
            cz, cr, cq = (d(_host(t)) for t in (cz, cr, cq))
        bz, z = _guarded(eng, shape, dtype, shift=shift)
        br, rh = _guarded(eng, shape, dtype, shift=shift)
        bo, out = _guarded(eng, shape, dtype, shift=shift)
        gz, grh = eng.raft_gru_zr(hx, packed_zr, cz, cr, h, z=z, rh=rh)
        assert gz.data_ptr() == z.data_ptr() and grh.data_ptr() == rh.data_ptr()
        got = eng.raft_gru_q(rh, packed_q, cq, z, h, x1=hx[:, Cc:], out=out)
        torch.cuda.synchronize()
        assert all(_guards_intact(b, n, shift=shift) for b in (bz, br, bo))
        assert np.array_equal(_bits(h), _bits(d(c.h))), "h was written"
        # out is h: the same bits
        h2 = d(c.h)
        assert eng.raft_gru_q(rh, packed_q, cq, z, h2, x1=hx[:, Cc:], out=h2) is h2
        assert np.array_equal(_bits(h2), _bits(got)), "out is h"
        return z, rh, got

    z, rh, got = run("plain", 0)
    hold(R, _host(z), ref.z, f"zr {name}: z", dtype)
    hold(R, _host(rh), ref.rh, f"zr {name}: r*h", dtype)
    hold(R, _host(got), ref, f"q {name}", dtype)
    # gate inputs of +-inf (and +-90) saturate to 0, 1 and -1 without a NaN
    zh, rhh, oh = _host(z), _host(rh), _host(got)
    assert np.isfinite(zh).all() and np.isfinite(rhh).all() and np.isfinite(oh).all()
    assert zh[0, 0, 0, 1] == 1.0 and zh[0, 1, 1, 2] == 0.0 and rhh[0, 0, 2, 3] == c.h[0, 0, 2, 3] and rhh[0, 2, 3, 4] == 0.0
    assert oh[0, 1, 1, 2] == c.h[0, 1, 1, 2] and zh[0, 3, 5, 9] == 1.0
    if name == "odd":
        for how, shift in (("slice", 0), ("shift", 1)):
            z2, rh2, got2 = run(how, shift)
            assert np.array_equal(_bits(z2), _bits(z)) and np.array_equal(_bits(rh2), _bits(rh)) and np.array_equal(_bits(got2), _bits(got)), how
        # each frame of the batch equals the one-frame call
        hx = _dev(eng, np.concatenate([c.h, c.x], axis=1), dtype)
        h, ctx = _dev(eng, c.h, dtype), _dev(eng, c.ctx, dtype)
        for f in range(c.B):
            cz, cr, cq = ctx[f:f + 1].split(Cc, dim=1)
            z1, rh1 = eng.raft_gru_zr(hx[f:f + 1], packed_zr, cz, cr, h[f:f + 1])
            o1 = eng.raft_gru_q(rh1, packed_q, cq, z1, h[f:f + 1], x1=hx[f:f + 1, Cc:])
            assert np.array_equal(_bits(z1), _bits(z)[f:f + 1]) and np.array_equal(_bits(rh1), _bits(rh)[f:f + 1]), f
            assert np.array_equal(_bits(o1), _bits(got)[f:f + 1]), f


# ---- refusals: before anything is launched, with no output byte touched -------------------------------------------------
def test_refusals_leave_every_byte_alone(eng):
    import torch
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((1 << 16,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((1 << 16,), SENTINEL32, dtype=torch.int32, device=eng.device)
    p, o = inp.data_ptr(), out.data_ptr()
    assert p % 16 == 0
    eng._bind_stream()
    n = 16 * 35

    def pack(w=p, bias=p, Cout=16, Cin=16, dtype=0, packed=o):
        return lib.vppx_raft_conv3x3_pack_dev(w, bias, Cout, Cin, dtype, packed, ctx)

    def conv(x0=p, s0=n, C0=16, x1=p, s1=n, C1=16, packed=p, Cout=16, B=2, H=5, W=7, relu=0, out_=o, so=n, dtype=0):
        return lib.vppx_raft_conv3x3_dt_dev(x0, s0, C0, x1, s1, C1, packed, Cout, B, H, W, relu, out_, so, dtype, ctx)

    def zr(x0=p, s0=2 * n, C0=32, x1=None, s1=0, C1=0, packed=p, cz=p, scz=n, cr=p, scr=n, h=p, sh=n, z=o, sz=n, rh=o + 4 * 2 * n, srh=n,
           B=2, Cc=16, H=5, W=7, dtype=0):
        return lib.vppx_raft_gru_zr_dt_dev(x0, s0, C0, x1, s1, C1, packed, cz, scz, cr, scr, h, sh, z, sz, rh, srh, B, Cc, H, W, dtype, ctx)

    def q(x0=p, s0=n, C0=16, x1=p, s1=n, C1=16, packed=p, cq=p, scq=n, z=p, sz=n, h=p, sh=n, out_=o, so=n, B=2, Cc=16, H=5, W=7, dtype=0):
        return lib.vppx_raft_gru_q_dt_dev(x0, s0, C0, x1, s1, C1, packed, cq, scq, z, sz, h, sh, out_, so, B, Cc, H, W, dtype, ctx)

    bad = "bad arguments"
    table = (
        # a NULL pointer
        (lambda: pack(w=None), INVALID, bad), (lambda: pack(packed=None), INVALID, bad),
        (lambda: conv(x0=None), INVALID, bad), (lambda: conv(x1=None), INVALID, bad), (lambda: conv(packed=None), INVALID, bad),
        (lambda: conv(out_=None), INVALID, bad),
        (lambda: zr(x0=None), INVALID, bad), (lambda: zr(packed=None), INVALID, bad), (lambda: zr(cz=None), INVALID, bad),
        (lambda: zr(cr=None), INVALID, bad), (lambda: zr(h=None), INVALID, bad), (lambda: zr(z=None), INVALID, bad), (lambda: zr(rh=None), INVALID, bad),
        (lambda: q(x0=None), INVALID, bad), (lambda: q(x1=None), INVALID, bad), (lambda: q(packed=None), INVALID, bad), (lambda: q(cq=None), INVALID, bad),
        (lambda: q(z=None), INVALID, bad), (lambda: q(h=None), INVALID, bad), (lambda: q(out_=None), INVALID, bad),
        # sizes <= 0
        (lambda: pack(Cout=0), INVALID, "C0 and Cout must be positive"), (lambda: pack(Cin=-16), INVALID, "must be positive"),
        (lambda: conv(B=0), INVALID, bad), (lambda: conv(H=0), INVALID, bad), (lambda: conv(W=-1), INVALID, bad),
        (lambda: conv(C0=0), INVALID, "must be positive"), (lambda: conv(C1=-16), INVALID, "C1 not negative"), (lambda: conv(Cout=0), INVALID, "must be positive"),
        (lambda: zr(B=0), INVALID, bad), (lambda: zr(Cc=0), INVALID, bad), (lambda: zr(H=-5), INVALID, bad), (lambda: q(W=0), INVALID, bad),
        (lambda: q(Cc=-16), INVALID, bad),
        # a frame stride below its tensor's size
        (lambda: conv(s0=n - 1), INVALID, "vppx_raft_conv3x3: x0_frame_stride 559 is less than 16 planes of 5x7"),
        (lambda: conv(s1=0), INVALID, "x1_frame_stride 0"), (lambda: conv(so=n - 1), INVALID, "out_frame_stride 559"),
        (lambda: zr(s0=2 * n - 1), INVALID, "vppx_raft_gru_zr: x0_frame_stride 1119 is less than 32 planes"),
        (lambda: zr(scz=1), INVALID, "cz_frame_stride 1"), (lambda: zr(scr=n - 1), INVALID, "cr_frame_stride"), (lambda: zr(sh=-n), INVALID, "h_frame_stride"),
        (lambda: zr(sz=n - 1), INVALID, "z_frame_stride"), (lambda: zr(srh=n - 1), INVALID, "rh_frame_stride"),
        (lambda: q(s1=n - 1), INVALID, "vppx_raft_gru_q: x1_frame_stride"), (lambda: q(scq=n - 1), INVALID, "cq_frame_stride"),
        (lambda: q(sz=n - 1), INVALID, "z_frame_stride"), (lambda: q(sh=n - 1), INVALID, "h_frame_stride"), (lambda: q(so=n - 1), INVALID, "out_frame_stride"),
        # a dtype other than the two
        (lambda: pack(dtype=2), INVALID, "vppx_raft_conv3x3_pack: dtype 2 is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)"),
        (lambda: conv(dtype=2), INVALID, "vppx_raft_conv3x3: dtype 2"), (lambda: zr(dtype=-1), INVALID, "vppx_raft_gru_zr: dtype -1"),
        (lambda: q(dtype=3), INVALID, "vppx_raft_gru_q: dtype 3"),
        # a packed buffer off its 16 bytes
        (lambda: pack(packed=o + 4), INVALID, "not 16-byte aligned"), (lambda: conv(packed=p + 8), INVALID, "not 16-byte aligned"),
        (lambda: zr(packed=p + 4), INVALID, "not 16-byte aligned"), (lambda: q(packed=p + 2), INVALID, "not 16-byte aligned"),
        # channel counts that are not built
        (lambda: pack(Cout=24), UNSUPPORTED, "multiples of 16"), (lambda: pack(Cin=8), UNSUPPORTED, "multiples of 16"),
        (lambda: pack(Cout=272), UNSUPPORTED, "up to 512 in and 256 out"), (lambda: pack(Cin=528), UNSUPPORTED, "up to 512 in"),
        (lambda: conv(C0=8, s0=8 * 35), UNSUPPORTED, "multiples of 16"), (lambda: conv(C1=24, s1=24 * 35), UNSUPPORTED, "multiples of 16"),
        (lambda: conv(Cout=40, so=40 * 35), UNSUPPORTED, "multiples of 16"), (lambda: conv(C0=512, s0=512 * 35), UNSUPPORTED, "up to 512 in"),
        (lambda: conv(Cout=272, so=272 * 35), UNSUPPORTED, "256 out"),
        (lambda: zr(Cc=8), UNSUPPORTED, "a hidden size of 8"), (lambda: zr(Cc=144, scz=144 * 35, scr=144 * 35, sh=144 * 35, sz=144 * 35, srh=144 * 35),
                                                                 UNSUPPORTED, "a hidden size of 144"),
        (lambda: q(Cc=8), UNSUPPORTED, "multiples of 16"), (lambda: q(Cc=272, scq=272 * 35, sz=272 * 35, sh=272 * 35, so=272 * 35), UNSUPPORTED, "256 out"),
        # more pixels than one launch takes
        (lambda: conv(B=1 << 12, H=1 << 10, W=1 << 10, s0=1 << 40, s1=1 << 40, so=1 << 40), UNSUPPORTED, "more than one launch takes"),
        (lambda: q(B=3, H=1 << 15, W=1 << 15, s0=1 << 40, s1=1 << 40, scq=1 << 40, sz=1 << 40, sh=1 << 40, so=1 << 40), UNSUPPORTED,
         "more than one launch takes"),
    )
    for k, (call, code, msg) in enumerate(table):
        rc = call()
        text = lib.vppx_last_error().decode()
        assert rc == code and msg in text, (k, rc, code, msg, text)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL32).all() and (inp.cpu().numpy() == 1.0).all()

    # through Engine
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=eng.device)            # noqa: E731
    packed = eng.raft_conv3x3_pack(f32(16, 32, 3, 3))
    with pytest.raises(ValueError, match="multiples of 16"):
        eng.raft_conv3x3_pack(f32(16, 24, 3, 3))
    with pytest.raises(ValueError, match=r"weight: expected a \[Cout,Cin,3,3\]"):
        eng.raft_conv3x3_pack(f32(16, 16, 1, 1))
    with pytest.raises(TypeError, match="float32 and bfloat16"):
        eng.raft_conv3x3_pack(f32(16, 16, 3, 3), dtype=torch.float16)
    with pytest.raises(ValueError, match="packed: "):
        eng.raft_conv3x3(f32(1, 16, 5, 7), packed, 16)                              # packed for 32 channels in
    with pytest.raises(ValueError, match="packed: "):
        eng.raft_conv3x3(f32(1, 32, 5, 7).bfloat16(), packed, 16)                   # packed for float32
    with pytest.raises(ValueError, match="x1: expected"):
        eng.raft_conv3x3(f32(1, 16, 5, 7), packed, 16, x1=f32(1, 16, 5, 8))
    with pytest.raises(ValueError, match="out: expected shape"):
        eng.raft_conv3x3(f32(1, 32, 5, 7), packed, 16, out=f32(1, 32, 5, 7))
    with pytest.raises(ValueError, match="cz: expected shape"):
        eng.raft_gru_zr(f32(1, 32, 5, 7), eng.raft_conv3x3_pack(f32(32, 32, 3, 3)), f32(1, 8, 5, 7), f32(1, 16, 5, 7), f32(1, 16, 5, 7))
    with pytest.raises(ValueError, match="z: expected shape"):
        eng.raft_gru_q(f32(1, 16, 5, 7), packed, f32(1, 16, 5, 7), f32(1, 16, 5, 6), f32(1, 16, 5, 7), x1=f32(1, 16, 5, 7))
    assert (out.cpu().numpy() == SENTINEL32).all()


# ---- the recording through fused_gru(conv=True) ----------------------------------------------------------------------------
def _conv_module(w, b, dtype, device):
    import torch
    m = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1)
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(w)), m.bias.copy_(torch.from_numpy(b))
    return m.to(device)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(R.RECORDED))
def test_fused_gru_reproduces_the_recording(eng, name, dtype):
    from vppstereo_amd.update import GruGlue
    g = R.load_recording()
    h0, ctx, xs, W = R.recorded_case(g, name)
    refs = R.recorded_ref(g, name, dtype)
    gru = SimpleNamespace(**{cv: _conv_module(W[f"{cv}_weight"], W[f"{cv}_bias"], dtype, eng.device) for cv in ("convz", "convr", "convq")})
    calls = []
    for cv in ("convz", "convr", "convq"):
        getattr(gru, cv).register_forward_hook(lambda m, i, o, cv=cv: calls.append(cv))
    rnd = (lambda a: R.to_bf16(a)) if dtype == "bfloat16" else (lambda a: a)
    glue = GruGlue()
    h = _dev(eng, rnd(h0), dtype)
    cz, cr, cq = _dev(eng, rnd(ctx), dtype).split(16, dim=1)
    x = [_dev(eng, rnd(a), dtype) for a in xs]
    packed = None
    for k, ref in enumerate(refs, start=1):
        new = glue.fused_gru(gru, h, cz, cr, cq, *x, conv=True)
        assert new.data_ptr() != h.data_ptr() and new.dtype == _tdtype(dtype)
        hold(R, _host(new), ref, f"recording {name} call {k}", dtype)
        if dtype == "float32":          # the reference's own h lies within the same limit of the same value
            assert (np.abs(_host(new).astype(F64) - g[f"{name}_h{k}"]) <= 2 * ref.limit).all()
        assert packed is None or glue._packed[id(gru)][1] is packed, "the weights were packed again"
        packed = glue._packed[id(gru)][1]
        h = new
    assert calls == [], "torch's convolutions ran"
    # a parameter written in place: packed again
    import torch
    with torch.no_grad():
        gru.convq.bias.add_(1.0)
    glue.fused_gru(gru, h, cz, cr, cq, *x, conv=True)
    assert glue._packed[id(gru)][1] is not packed


# ---- FusedUpdate(block, gru_conv=True) ---------------------------------------------------------------------------------
MOTION = 14                                  # the encoder's output channels: with the flow's two, 16


def _block(hidden, dtype, device, seed):
    """A stand-in BasicMultiUpdateBlock of seeded nn.Conv2ds; hidden = (gru08's, gru16's, gru32's) sizes."""
    import torch
    torch.manual_seed(seed)
    nn = torch.nn
    h08, h16, h32 = hidden
    gru = lambda hid, inp: SimpleNamespace(**{cv: nn.Conv2d(hid + inp, hid, 3, padding=1) for cv in ("convz", "convr", "convq")})    # noqa: E731
    blk = SimpleNamespace(n_gru_layers=3)
    blk.encoder = SimpleNamespace(convc1=nn.Conv2d(6, 8, 1), convc2=nn.Conv2d(8, 8, 3, padding=1), convf1=nn.Conv2d(2, 8, 7, padding=3),
                                  convf2=nn.Conv2d(8, 8, 3, padding=1), conv=nn.Conv2d(16, MOTION, 3, padding=1))
    blk.gru08, blk.gru16, blk.gru32 = gru(h08, MOTION + 2 + h16), gru(h16, h08 + h32), gru(h32, h16)
    blk.flow_head, blk.mask = nn.Conv2d(h08, 2, 3, padding=1), nn.Conv2d(h08, 9, 1)
    mods = list(vars(blk.encoder).values()) + [blk.flow_head, blk.mask] + [m for g in (blk.gru08, blk.gru16, blk.gru32) for m in vars(g).values()]
    with torch.no_grad():
        for m in mods:
            m.weight.mul_(2.0)
            m.to(device=device, dtype=_tdtype(dtype))
    return blk


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hidden", [(16, 16, 16), (16, 16, 8)])
def test_fused_update_with_the_convolutions(eng, hidden, dtype):
    """Two iterations of FusedUpdate(block, gru_conv=True).forward.  The motion features and what torch's own convolutions
    return are captured by forward hooks; from them the referee evaluates the three GRUs.  Within an iteration the bound of
    a GRU that ran on the kernel reaches the next level with its state (and the rounding of a bfloat16 store); a GRU that
    fell back is judged as tests/test_gpu_gru.py judges it, around what torch's convolutions returned, and hands the
    device's state on.  With gru32's hidden size 8, gru32 (24 channels in) and gru16 (40) fall back and gru08 (48) does not."""
    import torch
    from vppstereo_amd.update import FusedUpdate, GruGlue
    blk = _block(hidden, dtype, eng.device, 5901)
    seen = {}
    grus = {"gru08": blk.gru08, "gru16": blk.gru16, "gru32": blk.gru32}
    for tag, gru in grus.items():
        for cv in ("convz", "convr", "convq"):
            getattr(gru, cv).register_forward_hook(lambda m, i, o, key=f"{tag}.{cv}": seen.__setitem__(key, _host(o)))
    blk.encoder.conv.register_forward_hook(lambda m, i, o: seen.__setitem__("conv", _host(o)))
    fused = FusedUpdate(blk, gru_conv=True)
    rng = np.random.default_rng([5902, *hidden])
    rnd = (lambda a: R.to_bf16(a)) if dtype == "bfloat16" else (lambda a: a)
    sizes = [(9, 11)]
    for _ in range(2):
        sizes.append(tuple(G.pooled_size(v) for v in sizes[-1]))
    B = 2
    net_h = [rnd(np.tanh(rng.standard_normal((B, hidden[i]) + sizes[i])).astype(F32)) for i in range(3)]
    inp_h = [rnd(rng.standard_normal((B, 3 * hidden[i]) + sizes[i]).astype(F32)) for i in range(3)]
    flow_h = rnd((rng.standard_normal((B, 2) + sizes[0]) * 2.0).astype(F32))
    weights = {tag: {f"{cv}_{p}": getattr(getattr(gru, cv), p).detach().float().cpu().numpy() for cv in ("convz", "convr", "convq")
                     for p in ("weight", "bias")} for tag, gru in grus.items()}
    kernel = {"gru08": True, "gru16": hidden[2] == 16, "gru32": hidden[2] == 16}
    for tag, i, channels in (("gru32", 2, hidden[2] + hidden[1]), ("gru16", 1, hidden[1] + hidden[0] + hidden[2]),
                             ("gru08", 0, hidden[0] + MOTION + 2 + hidden[1])):
        assert GruGlue._conv_takes(grus[tag], hidden[i], channels) == kernel[tag], tag
    net = [_dev(eng, a, dtype) for a in net_h]
    inp = [list(_dev(eng, a, dtype).split(hidden[i], dim=1)) for i, a in enumerate(inp_h)]
    for it in range(2):
        seen.clear()
        corr = _dev(eng, rnd((rng.standard_normal((B, 6) + sizes[0]) * 2.0).astype(F32)), dtype)
        old = [_host(t) for t in net]
        net, mask, delta = fused(list(net), inp, corr, _dev(eng, flow_h, dtype))
        torch.cuda.synchronize()
        new = [_host(t) for t in net]
        assert ("gru08.convz" in seen, "gru16.convz" in seen, "gru32.convz" in seen) == tuple(not kernel[t] for t in ("gru08", "gru16", "gru32"))
        motion = rnd(np.maximum(seen["conv"], 0).astype(F32))           # relu(conv(.)) on its way into hx, in the working dtype
        state = [R._ns(a.astype(F64), np.zeros(a.shape)) for a in old]
        plan = (("gru32", 2, lambda: [(state[1].value, "pool2x", state[1].limit)]),
                ("gru16", 1, lambda: [(state[0].value, "pool2x", state[0].limit), (state[2].value, "interp", state[2].limit)]),
                ("gru08", 0, lambda: [(motion, "copy"), (flow_h, "copy"), (state[1].value, "interp", state[1].limit)]))
        for tag, i, sources in plan:
            Hh, Ww = sizes[i]
            what = f"iteration {it} {tag}"
            if kernel[tag]:
                x = R.stored(G.assemble(sources(), Hh, Ww), dtype)          # the x part of hx as the kernel reads it
                ref = R.gru(old[i], inp_h[i], [x.value], weights[tag], dtype, xs_limit=[x.limit])
                hold(R, new[i], ref, what, dtype)
                state[i] = R.stored(ref, dtype)
            else:
                cz, cr, cq = np.split(inp_h[i], 3, axis=1)
                _, _, ref = G.gru_ref(old[i], sources(), cz, cr, cq, seen[f"{tag}.convz"], seen[f"{tag}.convr"], seen[f"{tag}.convq"], 1.0)
                hold(G, new[i], ref, what, dtype)
                state[i] = R._ns(new[i].astype(F64), np.zeros(new[i].shape))
        assert delta.shape == (B, 2) + sizes[0] and mask.shape == (B, 9) + sizes[0]
        flow_h = rnd((flow_h + _host(delta)).astype(F32))
    for key, buf in fused._gates.items():            # one z and one r*h buffer per GRU on the kernel, kept from call to call
        assert key[1] in ("z", "rh") and kernel[{8: "gru08", 16: "gru16", 32: "gru32"}[key[0]]]
    assert len(fused._gates) == 2 * sum(kernel.values()) and sorted(fused._hx) == [8, 16, 32]
