"""PSMNet's stride-1 3-D convolutions on the convolution kernel (Engine.conv3d, vppx_conv3d_dt_dev) and FusedRegularization
against the float64 referee of tests/_psm3d_ref.py.

No atol.  Every finite float32 cell is held to the referee's limit, every bfloat16 cell to the band the single rounding of a
float32 inside that limit can reach.  A convolution's output is channels [0, Cout) of a [B, Cout + 2, D, H, W] buffer of sentinel
cells with guard cells around it, which must keep the sentinel bit for bit.  That the planted mistakes leave the limit on these
very arrays is asserted on the CPU in tests/test_psm3d_ref_cpu.py."""
import copy

import numpy as np
import pytest

import _psm3d_ref as P3
import _psm_ref as PR
from _cells import DTYPES, INVALID, SENTINEL16, SENTINEL32, UNSUPPORTED
from _cells import bits as _bits, dev as _dev, guarded as _guarded, guards_intact as _guards_intact, hold, host as _host, tdtype as _tdtype

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EXTRA = 2                                     # channels of the output's buffer behind the Cout the call writes
FACTOR = 4                                    # end to end: max |fused - f64| <= FACTOR * max |plain - f64| (tests/test_gpu_encoder_convs.py)
REGIMES = ("float32", "bfloat16", "autocast")


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
    return eng.conv3d_pack(_t(eng, w), _t(eng, bias), dtype=_tdtype(dtype))


def _run(eng, c, packed, dtype, res=None, relu=False, scale=1.0, shift=0, alias=False, x=None):
    """The case into channels [0, Cout) of a sentinel-filled [B, Cout + EXTRA, D, H, W] inside its guards.  alias: the residual is
    first copied into those channels and the call reads it from there, out being res itself."""
    import torch
    x = c.x if x is None else x
    B, _, D, H, W = x.shape
    buf, wide = _guarded(eng, (B, c.Cout + EXTRA, D, H, W), dtype, shift=shift)
    out = wide[:, :c.Cout]
    r = None if res is None else _dev(eng, res, dtype)
    if alias:
        out.copy_(r)
        r = out
    got = eng.conv3d(_dev(eng, x, dtype), packed, c.Cout, residual=r, relu=relu, scale=scale, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.dtype == _tdtype(dtype) and tuple(got.shape) == (B, c.Cout, D, H, W)
    raw = _bits(wide[:, c.Cout:])
    assert (raw == (SENTINEL16 if raw.dtype == np.int16 else SENTINEL32)).all(), f"a channel behind the {c.Cout} was written"
    assert _guards_intact(buf, B * (c.Cout + EXTRA) * D * H * W, shift=shift), "a guard cell was written"
    return got


# ---- the referee sweep ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cout", P3.SWEEP_COUTS)
@pytest.mark.parametrize("cin", P3.SWEEP_CINS)
@pytest.mark.parametrize("depth", P3.SWEEP_DEPTHS)
def test_the_convolution_equals_the_referee(eng, depth, cin, cout, dtype):
    """Workgroup tile 8 x 32 pixels and 64 channels of one plane (b, d); B = 2, so that a wrap between batch frames shows.  Every map
    under every epilogue, with out aliasing the residual, and with the base pointer one cell off its 16 bytes."""
    for H, W in P3.SWEEP_MAPS:
        c = P3.make(P3.SWEEP_B, cin, cout, depth, H, W, dtype)
        packed = _pack(eng, c.w, c.bias, dtype)
        pre = P3.conv3d_sum(c.x, c.w, c.bias, dtype)
        seen = {}
        for res, relu, scale in P3.EPILOGUES:
            ref = P3.conv3d(c.x, c.w, c.bias, dtype, res=c.res if res else None, relu=relu, scale=scale, pre=pre)
            got = _run(eng, c, packed, dtype, c.res if res else None, relu, scale)
            hold(PR, _host(got), ref, f"conv3d D={depth} {H}x{W} {cin} -> {cout} res={res} relu={relu} scale={scale}", dtype)
            seen[res, relu, scale] = _bits(got)
            if res:                                   # out aliased to res: the same bits
                assert np.array_equal(_bits(_run(eng, c, packed, dtype, c.res, relu, scale, alias=True)), seen[res, relu, scale])
        # an output one cell off its 16 bytes takes the cell route: the same bits
        shifted = _run(eng, c, packed, dtype, c.res, True, 0.25, shift=1)
        assert shifted.data_ptr() % 16 != 0 and np.array_equal(_bits(shifted), seen[True, True, 0.25])
        assert not np.array_equal(seen[True, False, 1.0], seen[False, False, 1.0])
        if (H, W) == (8, 32):
            got = _run(eng, c, packed, dtype, c.res, True, 0.25)
            assert got.data_ptr() % 16 == 0 and (got.stride(0) * got.element_size()) % 16 == 0                 # the 16-byte route


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(P3.CASES))
def test_the_named_cases_and_channel_slices(eng, name, dtype):
    """The cases tests/test_psm3d_ref_cpu.py plants its mistakes on; x and the residual as channel slices of wider tensors, frame
    strides above their size: the bits of the contiguous call."""
    import torch
    c = P3.case(name, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    got = _run(eng, c, packed, dtype, c.res, c.relu, c.scale)
    hold(PR, _host(got), P3.case_ref(c), name, dtype)

    def sliced(a):
        if a is None:
            return None
        wide = torch.zeros((a.shape[0], a.shape[1] + 3) + a.shape[2:], dtype=_tdtype(dtype), device=eng.device)
        wide[:, 2:2 + a.shape[1]] = _dev(eng, a, dtype)
        return wide[:, 2:2 + a.shape[1]]

    x, r = sliced(c.x), sliced(c.res)
    assert x.stride(0) > c.Cin * c.D * c.H * c.W and not x.is_contiguous()
    again = eng.conv3d(x, packed, c.Cout, residual=r, relu=c.relu, scale=c.scale)
    assert np.array_equal(_bits(again), _bits(got))


# ---- the packing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cout", [1, 32])
@pytest.mark.parametrize("cin", [16, 48])
def test_the_packed_bytes_are_those_of_the_permuted_weight(eng, cin, cout, dtype):
    import torch
    rng = np.random.default_rng([7631, cin, cout])
    w = rng.standard_normal((cout, cin, 3, 3, 3)).astype(F32)
    bias = rng.standard_normal(cout).astype(F32)
    for b in (bias, None):
        got = eng.conv3d_pack(_t(eng, w), _t(eng, b), dtype=_tdtype(dtype))
        want = eng.raft_conv_pack(_t(eng, P3.permuted(w)), _t(eng, b), dtype=_tdtype(dtype))
        assert got.dtype == torch.uint8 and got.numel() == want.numel() == eng.lib.vppx_conv3d_packed_bytes(cout, cin, 1 if dtype == "bfloat16" else 0)
        assert torch.equal(got, want)
    # a weight that is not contiguous is packed as its values
    wt = _t(eng, np.ascontiguousarray(w.transpose(1, 0, 2, 3, 4))).transpose(0, 1)
    want = eng.raft_conv_pack(_t(eng, P3.permuted(w)), _t(eng, bias), dtype=_tdtype(dtype))
    assert (cout == 1 or not wt.is_contiguous()) and torch.equal(eng.conv3d_pack(wt, _t(eng, bias), dtype=_tdtype(dtype)), want)


def test_pack_sizes_and_refusals(eng):
    import torch
    lib, ctx = eng.lib, eng.ctx.handle
    for cout, cin, dt in ((32, 64, 0), (1, 32, 1), (256, 160, 0), (80, 16, 1)):
        assert lib.vppx_conv3d_packed_bytes(cout, cin, dt) == lib.vppx_raft_conv_packed_bytes(cout, 3 * cin, 3, dt) > 0
    for cout, cin, dt in ((32, 0, 0), (32, -16, 0), (32, 8, 0), (32, 24, 0), (32, 176, 0), (0, 32, 0), (257, 32, 0), (32, 32, 2), (32, 32, -1)):
        assert lib.vppx_conv3d_packed_bytes(cout, cin, dt) == 0, (cout, cin, dt)
    w = torch.ones((1 << 16,), dtype=torch.float32, device=eng.device)
    out = torch.full((1 << 18,), SENTINEL32, dtype=torch.int32, device=eng.device)
    p, o = w.data_ptr(), out.data_ptr()
    eng._bind_stream()
    table = (
        (lambda: lib.vppx_conv3d_pack_dev(None, p, 32, 32, 0, o, ctx), INVALID, "vppx_conv3d_pack: bad arguments"),
        (lambda: lib.vppx_conv3d_pack_dev(p, p, 32, 32, 0, None, ctx), INVALID, "bad arguments"),
        (lambda: lib.vppx_conv3d_pack_dev(p, p, 32, 32, 2, o, ctx), INVALID, "dtype 2"),
        (lambda: lib.vppx_conv3d_pack_dev(p, p, 32, 0, 0, o, ctx), INVALID, "must be positive"),
        (lambda: lib.vppx_conv3d_pack_dev(p, p, 0, 32, 0, o, ctx), INVALID, "must be positive"),
        (lambda: lib.vppx_conv3d_pack_dev(p, p, 32, 8, 0, o, ctx), UNSUPPORTED, "multiples of 16 up to 160 in (3 x Cin up to 512)"),
        (lambda: lib.vppx_conv3d_pack_dev(p, p, 32, 176, 0, o, ctx), UNSUPPORTED, "176 input and 32 output channels"),
        (lambda: lib.vppx_conv3d_pack_dev(p, p, 257, 32, 0, o, ctx), UNSUPPORTED, "1 to 256 out"),
        (lambda: lib.vppx_conv3d_pack_dev(p, p, 32, 32, 0, o + 8, ctx), INVALID, "not 16-byte aligned"),
    )
    for k, (call, code, msg) in enumerate(table):
        rc = call()
        text = lib.vppx_last_error().decode()
        assert rc == code and msg in text, (k, rc, code, msg, text)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL32).all()
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=eng.device)            # noqa: E731
    with pytest.raises(ValueError, match=r"weight: expected a \[Cout,Cin,3,3,3\] tensor"):
        eng.conv3d_pack(f32(32, 32, 3, 3))
    with pytest.raises(ValueError, match=r"weight: expected a \[Cout,Cin,3,3,3\] tensor"):
        eng.conv3d_pack(f32(32, 32, 1, 3, 3))
    with pytest.raises(ValueError, match="weight: 8 -> 32 channels: multiples of 16 up to 160 in"):
        eng.conv3d_pack(f32(32, 8, 3, 3, 3))
    with pytest.raises(ValueError, match="176 -> 32 channels"):
        eng.conv3d_pack(f32(32, 176, 3, 3, 3))
    with pytest.raises(TypeError, match="dtype is"):
        eng.conv3d_pack(f32(32, 32, 3, 3, 3), dtype=torch.float16)
    with pytest.raises(ValueError, match="bias: expected shape"):
        eng.conv3d_pack(f32(32, 32, 3, 3, 3), f32(31))


# ---- NaN and batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_reaches_its_window_in_its_own_batch_frame(eng, dtype):
    c = P3.make(2, 16, 20, 3, 9, 33, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    run = lambda x: eng.conv3d(_dev(eng, x, dtype), packed, c.Cout, scale=0.25)           # noqa: E731  (no ReLU: it would turn -inf into 0)
    base = _bits(run(c.x))
    D, H, W = c.D, c.H, c.W
    counts = set()
    # the last plane of frame 0 (nothing of frame 1), the first plane of frame 1 (nothing of frame 0), corners, edges, the interior
    for b, ch, z, y, x in [(0, 3, D - 1, 4, 6), (1, 5, 0, 3, 31), (0, 15, 0, 0, 0), (1, 2, D - 1, H - 1, W - 1), (0, 9, 1, 4, 16), (0, 0, D - 1, 0, 32),
                           (1, 7, 0, 8, 5)]:
        for bad in (np.nan, np.inf):
            a = c.x.copy()
            a[b, ch, z, y, x] = bad
            got = run(a)
            hit = ~np.isfinite(_host(got))
            want = np.zeros_like(hit)
            want[b, :] = P3.nan_reach(D, H, W, z, y, x)[None]
            assert np.array_equal(hit, want), (bad, b, ch, z, y, x)
            assert not hit[1 - b].any() and np.array_equal(_bits(got)[~want], base[~want]), (bad, b, ch, z, y, x)
        counts.add(int(want[b, 0].sum()))
    assert counts == {8, 12, 18, 27}                 # a corner, an edge of the volume, a face, the interior
    # a NaN in the residual stays in its cell
    r = c.res.copy()
    r[1, 4, 0, 2, 2] = np.nan
    got = eng.conv3d(_dev(eng, c.x, dtype), packed, c.Cout, residual=_dev(eng, r, dtype))
    hit = np.isnan(_host(got))
    assert hit.sum() == 1 and hit[1, 4, 0, 2, 2]


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_frame_of_a_batch_has_the_bits_of_its_own_call(eng, dtype):
    c = P3.make(3, 32, 20, 3, 9, 33, dtype)
    packed = _pack(eng, c.w, c.bias, dtype)
    whole = _bits(eng.conv3d(_dev(eng, c.x, dtype), packed, c.Cout, residual=_dev(eng, c.res, dtype), relu=True))
    for b in range(3):
        one = _bits(eng.conv3d(_dev(eng, c.x[b:b + 1], dtype), packed, c.Cout, residual=_dev(eng, c.res[b:b + 1], dtype), relu=True))
        assert np.array_equal(one[0], whole[b]), b
    assert not np.array_equal(whole[0], whole[1])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_conv3d_refusals_leave_every_byte_alone(eng):
    import torch
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((1 << 16,), 1.0, dtype=torch.float32, device=eng.device)
    buf, outv = _guarded(eng, (1 << 16,), "float32")
    p, o = inp.data_ptr(), outv.data_ptr()
    eng._bind_stream()
    vol = 3 * 5 * 7
    nx, no = 16 * vol, 14 * vol

    def conv(x=p, sx=nx, Cin=16, packed=p, Cout=14, B=2, D=3, H=5, W=7, res=p, sr=no, relu=0, scale=1.0, out_=o, so=no, dtype=0):
        return lib.vppx_conv3d_dt_dev(x, sx, Cin, packed, Cout, B, D, H, W, res, sr, relu, scale, out_, so, dtype, ctx)

    bad = "bad arguments"
    big = 1 << 16
    table = (
        (lambda: conv(out_=None), INVALID, "vppx_conv3d: bad arguments"), (lambda: conv(scale=float("nan")), INVALID, "vppx_conv3d: the scale is not finite"),
        (lambda: conv(scale=float("inf"), x=None), INVALID, "not finite"), (lambda: conv(x=None), INVALID, bad), (lambda: conv(packed=None), INVALID, bad),
        (lambda: conv(D=0), INVALID, "B, D, H and W must be positive"), (lambda: conv(D=-3), INVALID, "B, D, H and W must be positive"),
        (lambda: conv(B=0), INVALID, bad), (lambda: conv(H=0), INVALID, bad), (lambda: conv(W=-1), INVALID, bad),
        (lambda: conv(D=0, dtype=2), INVALID, "B, D, H and W must be positive"), (lambda: conv(dtype=2), INVALID, "vppx_conv3d: dtype 2"),
        (lambda: conv(H=big, W=big), UNSUPPORTED, "map is more than the call takes"),
        (lambda: conv(D=big, H=big), UNSUPPORTED, "vppx_conv3d: a 65536x65536x7 volume is more than the call takes"),
        (lambda: conv(D=big, H=big, Cin=8), UNSUPPORTED, "volume is more than the call takes"),
        (lambda: conv(Cin=0), INVALID, "Cin and Cout must be positive"), (lambda: conv(Cout=0), INVALID, "Cin and Cout must be positive"),
        (lambda: conv(Cin=-16), INVALID, "must be positive"),
        (lambda: conv(Cin=8, sx=8 * vol), UNSUPPORTED, "multiples of 16 up to 160 in"), (lambda: conv(Cin=24, sx=24 * vol), UNSUPPORTED, "multiples of 16"),
        (lambda: conv(Cin=176, sx=176 * vol), UNSUPPORTED, "176 input and 14 output channels"),
        (lambda: conv(Cout=257, so=257 * vol, sr=257 * vol), UNSUPPORTED, "1 to 256 out"),
        (lambda: conv(Cin=8, packed=p + 8), UNSUPPORTED, "multiples of 16"), (lambda: conv(packed=p + 8), INVALID, "not 16-byte aligned"),
        (lambda: conv(packed=p + 8, sx=1), INVALID, "not 16-byte aligned"),
        (lambda: conv(sx=nx - 1), INVALID, "vppx_conv3d: x_frame_stride 1679 is less than 16 volumes of 3x5x7"), (lambda: conv(sx=0), INVALID, "x_frame_stride 0"),
        (lambda: conv(sx=nx - 1, sr=1, so=1), INVALID, "x_frame_stride 1679"),
        (lambda: conv(B=1 << 20, D=1 << 6, H=1 << 3, W=1 << 2, sx=16 << 11, sr=14 << 11, so=14 << 11), UNSUPPORTED, "B*D*H*W = 2147483648 cells"),
        (lambda: conv(B=1 << 20, D=1 << 6, H=1 << 3, W=1 << 2, sx=16 << 11, sr=1, so=1), UNSUPPORTED, "B*D*H*W"),
        (lambda: conv(sr=no - 1), INVALID, "vppx_conv3d: res_frame_stride 1469 is less than 14 volumes of 3x5x7"),
        (lambda: conv(sr=no - 1, so=1), INVALID, "res_frame_stride 1469"), (lambda: conv(sr=0), INVALID, "res_frame_stride 0"),
        (lambda: conv(so=no - 1), INVALID, "vppx_conv3d: out_frame_stride 1469 is less than 14 volumes of 3x5x7"),
        (lambda: conv(res=None, sr=0, so=14 * 35), INVALID, "out_frame_stride 490"),        # a 2-D frame is not enough
    )
    for k, (call, code, msg) in enumerate(table):
        rc = call()
        text = lib.vppx_last_error().decode()
        assert rc == code and msg in text, (k, rc, code, msg, text)
    torch.cuda.synchronize()
    assert _guards_intact(buf, 1 << 16) and (_bits(outv) == SENTINEL32).all() and (inp.cpu().numpy() == 1.0).all()
    # through Engine
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=eng.device)            # noqa: E731
    packed = eng.conv3d_pack(f32(14, 32, 3, 3, 3))
    x = f32(1, 32, 3, 5, 7)
    with pytest.raises(ValueError, match="x: expected a torch.float32 tensor with 5 dims"):
        eng.conv3d(f32(1, 32, 5, 7), packed, 14)
    with pytest.raises(TypeError, match="x is torch.float64"):
        eng.conv3d(x.double(), packed, 14)
    with pytest.raises(ValueError, match="packed: .* 32 -> 20 channels"):
        eng.conv3d(x, packed, 20)
    with pytest.raises(ValueError, match="packed: expected what conv3d_pack returns"):
        eng.conv3d(x, packed.float(), 14)
    with pytest.raises(ValueError, match="packed: .* 16 -> 14 channels"):
        eng.conv3d(f32(1, 16, 3, 5, 7), packed, 14)
    with pytest.raises(ValueError, match="residual: expected shape"):
        eng.conv3d(x, packed, 14, residual=f32(1, 14, 2, 5, 7))
    with pytest.raises(ValueError, match="residual: expected"):
        eng.conv3d(x, packed, 14, residual=f32(1, 14, 3, 5, 7).bfloat16())
    with pytest.raises(ValueError, match="out: expected shape"):
        eng.conv3d(x, packed, 14, out=f32(1, 14, 3, 5, 8))
    with pytest.raises(ValueError, match="every frame must be contiguous"):
        eng.conv3d(f32(1, 32, 3, 5, 14)[..., ::2], packed, 14)
    assert _guards_intact(buf, 1 << 16) and (_bits(outv) == SENTINEL32).all()


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------
def _wrapper_engine():
    """The Engine FusedRegularization launches on."""
    import torch
    from vppstereo_amd.corr import _engine
    return _engine(torch.device("cuda", torch.cuda.current_device()))


def _load(module, g, prefix=""):
    import torch
    state = {k[len(prefix):]: torch.from_numpy(np.asarray(g[k])) for k in g if k.startswith(prefix) and k[len(prefix):] in module.state_dict()}
    module.load_state_dict(state, strict=False)
    assert len(state) == sum(1 for k in module.state_dict() if not k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_wrapper_runs_the_recorded_dres1_block(dtype):
    """The reference's own Sequential(convbn_3d(16, 16, 3, 1, 1), ReLU, convbn_3d(16, 16, 3, 1, 1)) with `+ x`: 2 launches."""
    import torch
    import _raft_loop as L
    from vppstereo_amd.psmnet import FusedRegularization
    g = P3.load_recording()
    m = P3.standin(cin=16, c=16)
    _load(m.dres1, {k: g[k] for k in g.files}, "dres1.")
    eng = _wrapper_engine()
    wrapped = FusedRegularization(m.to(eng.device))
    x = g["dres1.x"]
    x = P3.to_bf16(x) if dtype == "bfloat16" else x
    xd = _dev(eng, x, dtype)
    with torch.no_grad(), L.LaunchSpy(eng, ("conv3d",)) as spy:
        got = wrapped._convbn(eng, m.dres1[2], wrapped._convbn(eng, m.dres1[0], xd, relu=True), residual=xd)
    assert len(spy.records) == 2 and got.dtype == _tdtype(dtype)
    ref = P3.dres1_block(x, g, "dres1.", dtype)
    hold(PR, _host(got), ref, "recorded dres1 block", dtype)
    hold(PR, L._np(spy.records[0].result), ref.hidden, "recorded dres1 block: the first convolution", dtype)
    if dtype == "float32":                        # the reference's own output lies within the same limit of the same value
        assert (np.abs(g["dres1.out"].astype(F64) - ref.value) <= 2 * ref.limit).all()
        assert (np.abs(_host(got).astype(F64) - g["dres1.out"]) <= 2 * ref.limit).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_wrapper_runs_the_recorded_hourglass(dtype):
    """The reference's own hourglass(16), called as dres3 calls it: conv2 with postsqu in front of its ReLU and conv4 are launches,
    the two stride-2 and the two transposed convolutions run in torch."""
    import torch
    import _raft_loop as L
    from vppstereo_amd.psmnet import FusedRegularization
    g = P3.load_recording()
    state = P3.hourglass_state(16)
    m = P3.standin(cin=16, c=16)
    _load(m.dres3, state)
    eng = _wrapper_engine()
    wrapped = FusedRegularization(m.to(eng.device))
    bf = (lambda a: P3.to_bf16(a)) if dtype == "bfloat16" else (lambda a: a)
    x, presqu, postsqu = bf(P3.hourglass_input()), bf(g["hg.presqu"]), bf(g["hg.postsqu"])
    ran = []
    hooks = [mod.register_forward_hook(lambda mod_, i, o, n=n: ran.append(n)) for n, mod in m.dres3.named_modules()
             if isinstance(mod, (torch.nn.Conv3d, torch.nn.ConvTranspose3d))]
    with torch.no_grad(), L.LaunchSpy(eng, ("conv3d",)) as spy:
        out, pre, post = wrapped._hourglass(eng, m.dres3, _dev(eng, x, dtype), _dev(eng, presqu, dtype), _dev(eng, postsqu, dtype))
    for h in hooks:
        h.remove()
    assert ran == ["conv1.0.0", "conv3.0.0", "conv5.0", "conv6.0"] and len(spy.records) == 2
    assert spy.records[0].kwargs["relu"] and np.array_equal(L._np(spy.records[0].kwargs["residual"]), postsqu)
    ref = P3.hourglass(x, state, "", dtype, presqu=presqu, postsqu=postsqu)
    for name, got in (("out", out), ("pre", pre), ("post", post)):
        assert got.dtype == _tdtype(dtype) and tuple(got.shape) == g[f"hg.{name}"].shape
        hold(PR, _host(got), getattr(ref, name), f"recorded hourglass: {name}", dtype)
        if dtype == "float32":                    # the reference's own output lies within the same limit of the same value
            assert (np.abs(g[f"hg.{name}"].astype(F64) - getattr(ref, name).value) <= 2 * getattr(ref, name).limit).all(), name
    # the two launches on the tensors the device had
    (c2, b2), (c4, b4) = (m.dres3.conv2[0], m.dres3.conv2[1]), (m.dres3.conv4[0][0], m.dres3.conv4[0][1])
    P3.check_conv3d_launch(spy.records[0], c2, b2, True, True, "recorded hourglass: conv2's launch")
    P3.check_conv3d_launch(spy.records[1], c4, b4, True, False, "recorded hourglass: conv4's launch")


def _plain(m, x, regime):
    import torch
    import _raft_loop as L
    with torch.no_grad(), L._autocast(x.device, regime == "autocast"):
        return m(x)


@pytest.mark.parametrize("regime", REGIMES)
def test_every_launch_of_the_wrapper_is_held_to_its_referee(regime):
    """A stand-in of the reference's structure with 16 / 32 channels on a [2,32,8,16,24] volume: 16 launches, each held to the
    referee on the tensors the device had; only the stride-2 and the transposed convolutions run in torch.  End to end
    max |fused - f64| <= 4 * max |plain - f64|, plain being the stand-in in torch operations on the device in the same regime."""
    import torch
    import _raft_loop as L
    from vppstereo_amd.psmnet import FusedRegularization
    eng = _wrapper_engine()
    m32 = P3.standin()
    m = (copy.deepcopy(m32).bfloat16() if regime == "bfloat16" else copy.deepcopy(m32)).to(eng.device)
    x32 = torch.randn((2, 32, 8, 16, 24), generator=torch.Generator().manual_seed(7702))
    x = (x32.bfloat16() if regime == "bfloat16" else x32).to(eng.device)
    wrapped = FusedRegularization(m)
    ran = []
    hooks = [mod.register_forward_hook(lambda mod_, i, o, n=n: ran.append(n)) for n, mod in m.named_modules()
             if isinstance(mod, (torch.nn.Conv3d, torch.nn.ConvTranspose3d))]
    with L._autocast(x.device, regime == "autocast"), L.LaunchSpy(eng, ("conv3d",)) as spy:
        out = wrapped(x)
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    want = torch.float32 if regime == "float32" else torch.bfloat16
    assert tuple(out.shape) == (2, 1, 8, 16, 24) and out.dtype == want and bool(torch.isfinite(out.float()).all())
    assert ran == [f"dres{k}.{c}" for k in (2, 3, 4) for c in ("conv1.0.0", "conv3.0.0", "conv5.0", "conv6.0")], ran
    assert len(spy.records) == wrapped.launches() == 16
    plan = P3.launch_plan(m)
    for k, (rec, (conv, bn, relu, has_res)) in enumerate(zip(spy.records, plan)):
        assert rec.args[0].dtype == want
        P3.check_conv3d_launch(rec, conv, bn, relu, has_res, f"{regime} launch {k}")
    # the sums in the epilogues are the reference's: dres1 + cost0, postsqu, cost1, cost2
    r = spy.records
    assert np.array_equal(L._np(r[3].kwargs["residual"]), L._np(r[1].result))                     # dres1(cost0) + cost0
    assert r[4].kwargs["residual"] is None and not np.array_equal(L._np(r[6].kwargs["residual"]), L._np(r[8].kwargs["residual"]))   # post1, post2
    assert np.array_equal(L._np(r[13].kwargs["residual"]), L._np(r[11].result))                   # classif2(out2) + cost1
    assert np.array_equal(L._np(r[15].kwargs["residual"]), L._np(r[13].result))                   # classif3(out3) + cost2
    # a second call gives the bits of a fresh wrapper
    with L._autocast(x.device, regime == "autocast"):
        again, fresh = wrapped(x), FusedRegularization(m)(x)
    assert np.array_equal(_bits(again), _bits(out)) and np.array_equal(_bits(fresh), _bits(out))
    # end to end
    with torch.no_grad():
        ref = copy.deepcopy(m).float().cpu().double()(x.float().cpu().double()).numpy()
    plain = _plain(m, x, regime)
    a, b = out.double().cpu().numpy(), plain.double().cpu().numpy()
    e_fused, e_plain = float(np.abs(a - ref).max()), float(np.abs(b - ref).max())
    print(f"{regime}: max |fused - f64| {e_fused:.3e}, max |plain - f64| {e_plain:.3e}, ratio {e_fused / e_plain:.3f}")
    assert e_plain > 0 and e_fused <= FACTOR * e_plain, f"{regime}: {e_fused:.3e} is more than {FACTOR} x {e_plain:.3e}"
    # a changed weight is seen
    with torch.no_grad():
        m.classif3[2].weight.mul_(2.0)
        m.dres0[0][1].running_var.add_(0.5)
    with L._autocast(x.device, regime == "autocast"):
        changed, fresh = wrapped(x), FusedRegularization(m)(x)
    assert not np.array_equal(_bits(changed), _bits(out)) and np.array_equal(_bits(changed), _bits(fresh))


def test_the_wrapper_refuses_training_mode_and_feeds_the_readout():
    """cost3 goes into Engine.psmnet_disparity as it is."""
    import torch
    from vppstereo_amd.psmnet import FusedRegularization
    eng = _wrapper_engine()
    m = P3.standin().to(eng.device)
    wrapped = FusedRegularization(m, dtype=torch.bfloat16)
    x = torch.randn((1, 32, 4, 8, 12), generator=torch.Generator().manual_seed(7703)).to(eng.device)
    cost3 = wrapped(x)
    assert cost3.dtype == torch.bfloat16 and tuple(cost3.shape) == (1, 1, 4, 8, 12)
    disp = eng.psmnet_disparity(cost3, 16, (32, 48))
    assert tuple(disp.shape) == (1, 32, 48) and bool(torch.isfinite(disp).all())
    m.dres0[2][1].train()
    with pytest.raises(RuntimeError, match="training mode"):
        wrapped(x)
    m.eval()
    with pytest.raises(ValueError, match="cost is"):
        wrapped(x[:, :, 0])
