"""The encoders' glue (norm_kernels.hip: the per-plane statistics and the norm / ReLU / residual-sum launch) against the
float64 referee of tests/_norm_ref.py.

No atol.  Every finite float32 cell is held to the referee's limit(), every bfloat16 cell to the band the single rounding of a
float32 inside that limit can reach; a cell that is not finite must have the referee's class.  Sentinel cells in front of
and behind every output must be intact.  The shapes are the smallest at which each route can go wrong: one cell, odd sizes
(cell by cell), whole 16-byte groups, a base one cell off alignment, a channel slice, and planes split over several
workgroups (chosen through vppx_norm_stats_pieces)."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import _norm_ref as N
from _cells import DTYPES, INVALID, SENTINEL32, UNSUPPORTED
from _cells import bits as _bits, dev as _dev, guarded as _guarded, guards_intact as _guards_intact, hold, host as _host

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SPLIT = (1, 2, 200, 201)                         # two planes of 40200 cells: three pieces of 13408, the last with 13384


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _case(name, dtype):
    """The input of a statistics case, float32 values (bfloat16-representable for a bfloat16 case)."""
    rng = np.random.default_rng([7701, len(name)])
    if name == "one":
        x = np.full((1, 1, 1, 1), 3.0, F32)
    elif name == "odd":
        x = (rng.standard_normal((2, 3, 5, 7)) * 2 + rng.standard_normal((2, 3, 1, 1))).astype(F32)
    elif name == "vec":
        x = (rng.standard_normal((1, 2, 8, 16)) * 0.5 - 1).astype(F32)
    elif name == "cancel":                     # a constant plane, and planes with |mean| >> std
        x = np.empty((1, 3, 4, 12), F32)
        x[0, 0] = 2.5
        x[0, 1] = 1000 + 4 * rng.integers(-1, 2, (4, 12))
        x[0, 2] = -3e4 + 256 * rng.integers(-1, 2, (4, 12))
    elif name == "nan":
        x = rng.standard_normal((2, 3, 5, 7)).astype(F32)
        x[0, 1, 2, 3] = np.nan
    elif name == "inf":
        x = rng.standard_normal((2, 3, 5, 7)).astype(F32)
        x[1, 0, 4, 6] = np.inf
    elif name == "split":
        x = (rng.standard_normal(SPLIT) * 3 + 10).astype(F32)
    return N.to_bf16(x) if dtype == "bfloat16" else x


CASES = ("one", "odd", "vec", "cancel", "nan", "inf", "split")


def _pieces(shape):
    from vppstereo_amd import _lib
    return _lib.load().vppx_norm_stats_pieces(shape[0] * shape[1], shape[2] * shape[3])


def _stats(eng, x):
    """raft_norm_stats into a guarded buffer -> the [B,C,2] tensor."""
    import torch
    B, Cc = x.shape[:2]
    buf, out = _guarded(eng, (B, Cc, 2), "float32")
    assert eng.raft_norm_stats(x, out=out) is out
    torch.cuda.synchronize()
    assert _guards_intact(buf, B * Cc * 2)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASES)
def test_statistics_and_the_norm_equal_the_referee(eng, name, dtype):
    import torch
    x = _case(name, dtype)
    assert (_pieces(x.shape) >= 3) == (name == "split")
    s = N.stats(x)
    xd = _dev(eng, x, dtype)
    st = _stats(eng, xd)
    hold(N, _host(st), N.stats_value(s), f"stats {name}", "float32")
    if name == "one":
        assert _host(st)[0, 0, 0] == 3.0 and _host(st)[0, 0, 1] == F32(1 / np.sqrt(1e-5))     # the variance is 0 exactly
    if name == "cancel":
        assert _host(st)[0, 0, 0] == 2.5 and _host(st)[0, 0, 1] == F32(1 / np.sqrt(1e-5))
    # the plain norm and norm + ReLU behind these statistics: the statistics' bounds go through the apply's
    for relu in (False, True):
        buf, out = _guarded(eng, x.shape, dtype)
        eng.raft_norm_apply(xd, st, relu=relu, out=out)
        torch.cuda.synchronize()
        assert _guards_intact(buf, x.size)
        hold(N, _host(out), N.apply(x, s, relu_inner=relu), f"apply {name} relu={relu}", dtype)
    if name in ("nan", "inf"):                 # the whole plane and no other
        got = _host(out)
        bad = np.isnan(got).all(axis=(2, 3))
        want = np.zeros(x.shape[:2], bool)
        want[(0, 1) if name == "nan" else (1, 0)] = True
        assert np.array_equal(bad, want) and np.isfinite(got[~want]).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["odd", "vec", "split"])
def test_alignment_and_slices_change_no_bit(eng, name, dtype):
    """One cell off alignment (the cell-by-cell route) and a channel slice of a wider tensor (a frame stride above C*H*W)
    give the bits of the aligned, contiguous call: statistics, and the apply with a residual."""
    import torch
    x = _case(name, dtype)
    B, Cc, H, W = x.shape
    xd = _dev(eng, x, dtype)
    rd = _dev(eng, x[:, ::-1].copy(), dtype)           # the residual: the channels in reverse order
    st = _stats(eng, xd)
    want = _bits(eng.raft_norm_apply(xd, st, residual=rd))

    def shifted(t):
        flat = torch.zeros((t.numel() + 1,), dtype=t.dtype, device=eng.device)
        v = flat[1:].view(t.shape)
        v.copy_(t)
        return v

    def sliced(t):
        wide = torch.zeros((B, Cc + 2, H, W), dtype=t.dtype, device=eng.device)
        wide[:, 1:1 + Cc] = t
        return wide[:, 1:1 + Cc]

    for how in (shifted, sliced):
        xs, rs = how(xd), how(rd)
        assert how is shifted or xs.stride(0) == (Cc + 2) * H * W
        st2 = _stats(eng, xs)
        assert np.array_equal(_bits(st2), _bits(st)), (name, how.__name__)
        out = how(torch.zeros_like(xd))
        eng.raft_norm_apply(xs, st2, residual=rs, out=out)
        assert np.array_equal(_bits(out), want), (name, how.__name__)


def test_split_planes_leave_nothing_behind(eng):
    """The split route twice, with a call of another shape and dtype between: the same bits, so no partial sum of an earlier
    call is read and nothing depends on dispatch order."""
    B, Cc, H, W = SPLIT
    pieces = _pieces(SPLIT)
    per = -(-H * W // pieces)
    chunk = -(-per // 16) * 16                         # include/vppx.h: ceil(H*W / pieces), rounded up to whole 16 cells
    assert pieces >= 3 and 0 < H * W - (pieces - 1) * chunk < chunk and B * Cc * H * W < 1 << 20
    xd = _dev(eng, _case("split", "float32"))
    first = _bits(_stats(eng, xd))
    other = _case("split", "bfloat16")[:, :, :150] * F32(-2)
    assert _pieces(other.shape) not in (1, pieces)
    od = _dev(eng, other, "bfloat16")
    hold(N, _host(_stats(eng, od)), N.stats_value(N.stats(other)), "stats between", "float32")
    _stats(eng, _dev(eng, _case("odd", "float32")))
    assert np.array_equal(_bits(_stats(eng, xd)), first)


def _apply_inputs(shape, dtype):
    rng = np.random.default_rng([7702, *shape])
    B, Cc = shape[:2]
    q = (lambda a: N.to_bf16(a.astype(F32))) if dtype == "bfloat16" else (lambda a: a.astype(F32))
    f = lambda *s: rng.standard_normal(s).astype(F32)                                   # noqa: E731
    a = SimpleNamespace(x=q(f(*shape) * 2 + 1), res=q(f(*shape)))
    a.stats = np.stack([f(B, Cc), np.abs(f(B, Cc)) + F32(0.25)], axis=-1)
    a.res_stats = np.stack([f(B, Cc), np.abs(f(B, Cc)) + F32(0.25)], axis=-1)
    a.weight, a.bias, a.res_weight, a.res_bias = f(Cc) * 1.5, f(Cc), f(Cc) * 1.5, f(Cc)
    a.x[0, 0, 0, 0], a.res[-1, -1, -1, -1] = np.nan, np.inf
    return a


def _given(st):
    """Statistics handed in as float32 numbers: the kernel reads exactly these, so they carry no bound."""
    st = np.asarray(st, F64)
    st = st[None] if st.ndim == 2 else st
    return SimpleNamespace(mean=st[..., 0], rstd=st[..., 1], dmean=np.zeros(st.shape[:2]), drstd=np.zeros(st.shape[:2]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 2, 8, 16), (1, 1, 70, 64)])
def test_apply_every_option(eng, shape, dtype):
    """weight / bias, the inner ReLU, no residual / a residual / one with statistics / with statistics and weights, and one
    set of statistics for every frame (stride 0) -- 2 x 2 x 4 x 2 launches; then in place over x and over the residual.
    (1,1,70,64): more than one workgroup per plane, the last part-filled."""
    import torch
    a = _apply_inputs(shape, dtype)
    d = SimpleNamespace(x=_dev(eng, a.x, dtype), res=_dev(eng, a.res, dtype), **{k: _dev(eng, getattr(a, k)) for k in
                        ("stats", "res_stats", "weight", "bias", "res_weight", "res_bias")})
    for affine, relu, rmode, shared in itertools.product((False, True), (False, True), range(4), (False, True)):
        st, rst = (a.stats[0], a.res_stats[0]) if shared else (a.stats, a.res_stats)
        dst, drst = (d.stats[0].contiguous(), d.res_stats[0].contiguous()) if shared else (d.stats, d.res_stats)
        kw = dict(weight=d.weight, bias=d.bias) if affine else {}
        rkw = dict(weight=a.weight, bias=a.bias) if affine else {}
        if rmode >= 1:
            kw["residual"], rkw["res"] = d.res, a.res
        if rmode >= 2:
            kw["residual_stats"], rkw["res_stats"] = drst, _given(rst)
        if rmode == 3:
            kw.update(residual_weight=d.res_weight, residual_bias=d.res_bias)
            rkw.update(res_weight=a.res_weight, res_bias=a.res_bias)
        buf, out = _guarded(eng, shape, dtype)
        eng.raft_norm_apply(d.x, dst, relu=relu, out=out, **kw)
        torch.cuda.synchronize()
        assert _guards_intact(buf, a.x.size)
        what = f"apply {shape} affine={affine} relu={relu} residual={rmode} shared={shared}"
        hold(N, _host(out), N.apply(a.x, _given(st), relu_inner=relu, **rkw), what, dtype)
        if rmode >= 1 and not shared:
            for target in ("x", "res"):        # out = x, out = res: every cell is read before it is written
                xs, rs = d.x.clone(), d.res.clone()
                t = xs if target == "x" else rs
                assert eng.raft_norm_apply(xs, dst, relu=relu, **{**kw, "residual": rs}, out=t) is t
                assert np.array_equal(_bits(t), _bits(out)), (what, target)
                assert np.array_equal(_bits(rs if target == "x" else xs), _bits(d.res if target == "x" else d.x))


def test_engine_checks(eng):
    import torch
    x = torch.zeros((2, 3, 5, 7), device=eng.device)
    st = eng.raft_norm_stats(x)
    assert st.shape == (2, 3, 2) and st.dtype == torch.float32
    with pytest.raises(TypeError, match="float16"):
        eng.raft_norm_stats(x.half())
    with pytest.raises(TypeError, match="float16"):
        eng.raft_norm_apply(x.half(), st)
    with pytest.raises(ValueError, match="residual"):
        eng.raft_norm_apply(x, st, residual=x[:, :2])
    with pytest.raises(ValueError, match="residual"):
        eng.raft_norm_apply(x, st, residual=x.bfloat16())
    with pytest.raises(ValueError, match="stats"):
        eng.raft_norm_apply(x, st[:, :2].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        eng.raft_norm_stats(x.permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match="weight"):
        eng.raft_norm_apply(x, st, weight=torch.ones(4, device=eng.device), bias=torch.ones(3, device=eng.device))
    from vppstereo_amd import _lib
    with pytest.raises(_lib.VppxError, match="goes with its bias"):
        eng.raft_norm_apply(x, st, weight=torch.ones(3, device=eng.device))
    with pytest.raises(_lib.VppxError, match="eps"):
        eng.raft_norm_stats(x, eps=0.0)


def test_refusals_leave_every_byte_alone(eng):
    import torch
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((8192,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((8192,), SENTINEL32, dtype=torch.int32, device=eng.device)
    p, o = inp.data_ptr(), out.data_ptr()
    eng._bind_stream()

    def stats(x=p, sx=105, B=2, Cc=3, H=5, W=7, eps=1e-5, st=o, dtype=0, c=ctx):
        return lib.vppx_raft_norm_stats_dt_dev(x, sx, B, Cc, H, W, eps, st, dtype, c)

    def apply(x=p, sx=105, st=p, sst=6, w=None, b=None, relu=1, res=None, sres=105, rst=None, srst=6, rw=None, rb=None, out_=o, so=105,
              B=2, Cc=3, H=5, W=7, dtype=0, c=ctx):
        return lib.vppx_raft_norm_apply_dt_dev(x, sx, st, sst, w, b, relu, res, sres, rst, srst, rw, rb, out_, so, B, Cc, H, W, dtype, c)

    NO_DEVICE = -7
    bad = "bad arguments"
    table = (
        (lambda: stats(c=None), NO_DEVICE, "context is NULL"), (lambda: apply(c=None), NO_DEVICE, "context is NULL"),
        # a NULL tensor
        (lambda: stats(x=None), INVALID, bad), (lambda: stats(st=None), INVALID, bad),
        (lambda: apply(x=None), INVALID, bad), (lambda: apply(st=None), INVALID, bad), (lambda: apply(out_=None), INVALID, bad),
        # sizes <= 0
        (lambda: stats(B=0), INVALID, bad), (lambda: stats(Cc=-1), INVALID, bad), (lambda: stats(H=0), INVALID, bad),
        (lambda: stats(W=0), INVALID, bad),
        (lambda: apply(B=0), INVALID, bad), (lambda: apply(Cc=0), INVALID, bad), (lambda: apply(H=-5), INVALID, bad),
        (lambda: apply(W=0), INVALID, bad),
        # a frame stride below its tensor
        (lambda: stats(sx=104), INVALID, "vppx_raft_norm_stats: x_frame_stride 104 is less than 3 planes of 5x7"),
        (lambda: apply(sx=104), INVALID, "vppx_raft_norm_apply: x_frame_stride 104 is less than 3 planes of 5x7"),
        (lambda: apply(so=0), INVALID, "out_frame_stride 0"), (lambda: apply(res=p, sres=104), INVALID, "res_frame_stride 104"),
        # a stats stride other than 0 or 2*C
        (lambda: apply(sst=5), INVALID, "vppx_raft_norm_apply: stats_frame_stride 5 is neither 0 (one set for every frame) nor 2*C = 6"),
        (lambda: apply(sst=12), INVALID, "stats_frame_stride 12"), (lambda: apply(sst=-6), INVALID, "stats_frame_stride -6"),
        (lambda: apply(res=p, rst=p, srst=7), INVALID, "res_stats_frame_stride 7"),
        # a dtype other than the two
        (lambda: stats(dtype=2), INVALID, "vppx_raft_norm_stats: dtype 2 is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)"),
        (lambda: apply(dtype=-1), INVALID, "vppx_raft_norm_apply: dtype -1"),
        # eps not finite or <= 0
        (lambda: stats(eps=0.0), INVALID, "eps 0 is not a positive finite number"), (lambda: stats(eps=-1e-5), INVALID, "eps -1e-05"),
        (lambda: stats(eps=float("inf")), INVALID, "eps inf"), (lambda: stats(eps=float("nan")), INVALID, "eps nan"),
        # weight without bias or the reverse
        (lambda: apply(w=p), INVALID, "a weight goes with its bias"), (lambda: apply(b=p), INVALID, "a weight goes with its bias"),
        (lambda: apply(res=p, rst=p, rw=p), INVALID, "a weight goes with its bias"),
        (lambda: apply(res=p, rst=p, rb=p), INVALID, "a weight goes with its bias"),
        # res_stats or res_weight without res, res_weight without res_stats
        (lambda: apply(rst=p), INVALID, "res_stats or res_weight without res"),
        (lambda: apply(rw=p, rb=p), INVALID, "res_stats or res_weight without res"),
        (lambda: apply(res=p, rw=p, rb=p), INVALID, "res_weight without res_stats"),
        # too many cells for one launch
        (lambda: stats(sx=1 << 40, H=1 << 16, W=1 << 16), UNSUPPORTED, "a 65536x65536 map is more than the call takes"),
        (lambda: apply(sx=1 << 62, so=1 << 62, B=1 << 20, Cc=1 << 10, H=1 << 15, W=1 << 15, sst=0), UNSUPPORTED,
         "workgroups, more than one launch takes"),
        (lambda: stats(sx=1 << 62, B=1 << 20, Cc=1 << 11, H=1 << 15, W=1 << 15), UNSUPPORTED, "more workgroups than one launch takes"),
    )
    for k, (call, code, text) in enumerate(table):
        assert call() == code, (k, lib.vppx_last_error())
        assert text in lib.vppx_last_error().decode(), (k, text, lib.vppx_last_error())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL32).all()) and bool((inp == 1.0).all())
    # and the same context still works
    assert stats(st=o) == 0 and apply(out_=o + 4096) == 0
    torch.cuda.synchronize()
    assert _host(out.view(torch.float32)[:12]).reshape(6, 2).tolist() == [[1.0, float(F32(1 / np.sqrt(1e-5)))]] * 6


PLAN = (((1, 2, 200, 201), "float32"), ((2, 3, 5, 7), "bfloat16"), ((1, 2, 8, 16), "float32"), ((1, 3, 150, 201), "bfloat16"),
        ((1, 1, 1, 1), "float32"), ((2, 3, 5, 7), "float32"), ((1, 2, 200, 201), "bfloat16"), ((4, 16, 3, 4), "bfloat16"))


def test_one_context_through_unlike_calls(eng):
    """One context through a plan of unlike shapes and dtypes, each a ResidualBlock's tail: statistics of y and of a
    downsample path's r, then relu(norm(r) + relu(norm(y))), held to the referee with the statistics' own bounds."""
    import torch
    seen = set()
    for k, (shape, dtype) in enumerate(PLAN):
        rng = np.random.default_rng([7703, k])
        q = (lambda a: N.to_bf16(a.astype(F32))) if dtype == "bfloat16" else (lambda a: a.astype(F32))
        y, r = q(rng.standard_normal(shape) * 2 + 0.5), q(rng.standard_normal(shape) - 1)
        yd, rd = _dev(eng, y, dtype), _dev(eng, r, dtype)
        sy, sr = eng.raft_norm_stats(yd), eng.raft_norm_stats(rd, eps=1e-3)
        buf, out = _guarded(eng, shape, dtype)
        eng.raft_norm_apply(yd, sy, residual=rd, residual_stats=sr, out=out)
        torch.cuda.synchronize()
        assert _guards_intact(buf, y.size)
        hold(N, _host(out), N.apply(y, N.stats(y), res=r, res_stats=N.stats(r, eps=1e-3)), f"plan {k} {shape}", dtype)
        seen.add(_pieces(shape))
    assert len(seen) >= 3                      # one piece, and two different splits
