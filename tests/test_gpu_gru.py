"""The update block's glue (gru_kernels.hip: the assembly of hx, the reset gate over hx, the GRU update) and
vppstereo_amd.update.FusedUpdate against the float64 referee of tests/_gru_ref.py.

No atol.  Every finite float32 cell is held to the referee's limit(), every bfloat16 cell to the band the single
rounding of a float32 inside that limit can reach, with an expf within DEVICE_EXP_ULPS of the true value
(tests/test_gpu_handoff_ref.py says where the figure is from); a cell that is not finite must have the referee's class.
Sentinel cells in front of and behind every output must be intact.  What the cases reach, and that the planted mistakes
leave the limit on these very arrays, is asserted on the CPU in tests/test_gru_ref_cpu.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import _gru_ref as R
from _cells import DTYPES, INVALID, SENTINEL16, SENTINEL32, UNSUPPORTED
from _cells import bits as _bits, dev as _dev, guarded as _guarded, guards_intact as _guards_intact, hold, host as _host, tdtype as _tdtype

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DEVICE_EXP_ULPS = 1.0
_REFS = {}


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


# ---- the assembly of hx -------------------------------------------------------------------------------------------------
def _assemble_ref(name, dtype):
    if ("asm", name, dtype) not in _REFS:
        c = R.assemble_case(name, dtype)
        _REFS["asm", name, dtype] = (c, R.assemble_ref(c))
    return _REFS["asm", name, dtype]


def _sources(eng, c, how):
    """The case's sources on the device.  how = "parent": the view parent[:, :C*Hs*Ws] of the padded parent (the frame
    stride of the case); "slice": channels 1 .. C of a [B,C+2,Hs,Ws] tensor (the base Hs*Ws cells into it);
    "shift": a contiguous tensor one cell into its buffer."""
    import torch
    out = []
    for s in c.sources:
        parent, Cc, Hs, Ws, mode = s
        B = parent.shape[0]
        if how == "parent":
            t = _dev(eng, parent, c.dtype)[:, :Cc * Hs * Ws].view(B, Cc, Hs, Ws)
        elif how == "slice":
            wide = np.zeros((B, Cc + 2, Hs, Ws), F32)
            wide[:, 1:1 + Cc] = R.source_view(s)
            t = _dev(eng, wide, c.dtype)[:, 1:1 + Cc]
        else:
            flat = torch.zeros((B * Cc * Hs * Ws + 1,), dtype=_tdtype(c.dtype), device=eng.device)
            t = flat[1:].view(B, Cc, Hs, Ws)
            t.copy_(_dev(eng, R.source_view(s), c.dtype))
        out.append((t, mode))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(R.ASSEMBLE_CASES))
def test_assemble_equals_the_referee(eng, name, dtype):
    import torch
    c, ref = _assemble_ref(name, dtype)
    shape = (c.B, c.hx_channels, c.H, c.W)
    buf, out = _guarded(eng, shape, dtype)
    assert out.data_ptr() % 16 == 0
    got = eng.raft_gru_assemble(_sources(eng, c, "parent"), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.dtype == _tdtype(dtype)
    host = _host(got)
    hold(R, host[:, :c.channels], ref, f"assemble {name}", dtype)
    assert _guards_intact(buf, int(np.prod(shape)))
    bits = _bits(got)
    if c.hx_channels > c.channels:      # channels behind the sources' are not written
        assert (bits[:, c.channels:] == (SENTINEL16 if dtype == "bfloat16" else SENTINEL32)).all()
    # a copied source arrives bit for bit
    C0 = c.sources[0][1]
    assert np.array_equal(bits[:, :C0], _bits(_sources(eng, c, "parent")[0][0]))
    # the same data through channel slices of wider tensors, and through tensors and an output one cell off their
    # buffers' boundaries, which takes the cell-by-cell route: the same bits
    for how, shift in (("slice", 0), ("shift", 1)):
        buf2, out2 = _guarded(eng, shape, dtype, shift=shift)
        srcs = _sources(eng, c, how)
        if how == "shift":
            assert out2.data_ptr() % 16 != 0 and all(t.data_ptr() % 16 != 0 for t, _ in srcs)
        elif c.H * c.W % 2:
            assert srcs[0][0].data_ptr() % 16 != 0
        eng.raft_gru_assemble(srcs, out=out2)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out2)[:, :c.channels], bits[:, :c.channels]), (name, how)
        assert _guards_intact(buf2, int(np.prod(shape)), shift=shift)
    if c.hx_channels == c.channels:     # without out= the size comes from the copied source
        fresh = eng.raft_gru_assemble(_sources(eng, c, "parent"))
        assert fresh.shape == shape and fresh.is_contiguous() and np.array_equal(_bits(fresh), bits)


def test_assemble_frames_of_a_batch_equal_one_frame_calls(eng):
    for dtype in DTYPES:
        c, _ = _assemble_ref("odd_a", dtype)
        srcs = _sources(eng, c, "parent")
        both = _bits(eng.raft_gru_assemble(srcs))
        assert not np.array_equal(both[0], both[1])
        for f in range(c.B):
            one = eng.raft_gru_assemble([(t[f:f + 1], m) for t, m in srcs])
            assert np.array_equal(_bits(one), both[f:f + 1]), (dtype, f)


# ---- the gates ----------------------------------------------------------------------------------------------------------
def _gate_ref(name, dtype):
    if ("gate", name, dtype) not in _REFS:
        c = R.gate_case(name, dtype)
        _REFS["gate", name, dtype] = (c, R.reset(c.ar, c.cr, c.h, DEVICE_EXP_ULPS), R.update(c.az, c.cz, c.aq, c.cq, c.h, DEVICE_EXP_ULPS))
    return _REFS["gate", name, dtype]


def _padded(eng, a, dtype, stride):
    """a [B,C,H,W] as a view of a [B,stride] buffer: frames `stride` cells apart."""
    B, n = a.shape[0], int(np.prod(a.shape[1:]))
    parent = np.zeros((B, stride), F32)
    parent[:, :n] = a.reshape(B, n)
    return _dev(eng, parent, dtype)[:, :n].view(*a.shape)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(R.GATE_CASES))
def test_reset_and_update_equal_the_referee(eng, name, dtype):
    import torch
    c, ref_r, ref_u = _gate_ref(name, dtype)
    Cc = c.C
    d = lambda a: _dev(eng, a, dtype)                                                     # noqa: E731
    az, ar, aq, h = d(c.az), d(c.ar), d(c.aq), d(c.h)
    cz, cr, cq = d(c.c).split(Cc, dim=1)                     # views of one [B,3C,H,W] tensor: frames 3C*H*W apart
    assert not cr.is_contiguous() and cr.stride(0) == 3 * Cc * c.H * c.W
    shape = (c.B, Cc + 2, c.H, c.W)
    buf, hx = _guarded(eng, shape, dtype)
    hx.copy_(torch.cat([h, d(c.x)], dim=1))
    x_before = _bits(hx[:, Cc:])
    assert eng.raft_gru_reset(ar, cr, h, hx) is hx
    torch.cuda.synchronize()
    hold(R, _host(hx[:, :Cc]), ref_r, f"reset {name}", dtype)
    assert np.array_equal(_bits(hx[:, Cc:]), x_before), "reset touched the x part of hx"
    assert _guards_intact(buf, int(np.prod(shape)))
    assert np.array_equal(_bits(h), _bits(d(c.h))), "reset wrote h"
    reset_bits = _bits(hx[:, :Cc])

    buf_o, out = _guarded(eng, c.h.shape, dtype)
    got = eng.raft_gru_update(az, cz, aq, cq, h, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    hold(R, _host(got), ref_u, f"update {name}", dtype)
    assert _guards_intact(buf_o, c.h.size)
    update_bits = _bits(got)
    cls = R.classes(_host(got))
    assert (cls == 1).any() and (cls == 2).any()
    # a fresh output, and out is h: the same bits
    assert np.array_equal(_bits(eng.raft_gru_update(az, cz, aq, cq, h)), update_bits)
    h2 = d(c.h)
    assert eng.raft_gru_update(az, cz, aq, cq, h2, out=h2) is h2
    assert np.array_equal(_bits(h2), update_bits), "out is h"

    # every tensor one cell off its buffer's boundary (the cell-by-cell route), and every tensor in frames 112 cells apart
    # (16-byte groups with a last group that is not whole when C*H*W is odd): the same bits
    def shifted(a):
        flat = torch.zeros((a.numel() + 1,), dtype=_tdtype(dtype), device=eng.device)
        t = flat[1:].view(*a.shape)
        t.copy_(a)
        assert t.data_ptr() % 16 != 0
        return t

    n = Cc * c.H * c.W
    stride = (n + 15) // 16 * 16 + 16
    routes = {"shift": shifted, "padded": lambda a: _padded(eng, _host(a), dtype, stride * (a.shape[1] // Cc))}
    for how, mk in routes.items():
        hx2 = mk(torch.cat([h, d(c.x)], dim=1)) if how == "shift" else _padded(eng, np.concatenate([c.h, c.x], axis=1), dtype, 2 * stride)
        eng.raft_gru_reset(mk(ar), mk(cr), mk(h), hx2)
        assert np.array_equal(_bits(hx2[:, :Cc]), reset_bits) and np.array_equal(_bits(hx2[:, Cc:]), x_before), how
        o2 = mk(h)
        eng.raft_gru_update(mk(az), mk(cz), mk(aq), mk(cq), o2, out=o2)
        assert np.array_equal(_bits(o2), update_bits), how


# ---- refusals: before anything is launched, with no output byte touched -------------------------------------------------
def test_refusals_leave_every_byte_alone(eng):
    import torch
    from vppstereo_amd import _lib
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((8192,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((8192,), SENTINEL32, dtype=torch.int32, device=eng.device)
    p, o = inp.data_ptr(), out.data_ptr()
    eng._bind_stream()
    COPY, POOL, INTERP = 0, 1, 2

    def asm(srcs=((p, 70, 2, 5, 7, COPY),), n=None, B=1, H=5, W=7, hx=o, hxc=4, dtype=0, null_sources=False):
        arr = (_lib.VppxGruSource * max(len(srcs), 1))()
        for k, s in enumerate(srcs):
            arr[k] = _lib.VppxGruSource(*s)
        return lib.vppx_raft_gru_assemble_dt_dev(ctx, None if null_sources else arr, len(srcs) if n is None else n, B, H, W, hx, hxc, dtype)

    def reset(ar=p, sar=105, cr=p, scr=105, h=p, sh=105, hx=o, shx=175, B=2, Cc=3, H=5, W=7, hxc=5, dtype=0):
        return lib.vppx_raft_gru_reset_dt_dev(ctx, ar, sar, cr, scr, h, sh, hx, shx, B, Cc, H, W, hxc, dtype)

    def update(az=p, saz=105, cz=p, scz=105, aq=p, saq=105, cq=p, scq=105, h=p, sh=105, out_=o, so=105, B=2, Cc=3, H=5, W=7, dtype=0):
        return lib.vppx_raft_gru_update_dt_dev(ctx, az, saz, cz, scz, aq, saq, cq, scq, h, sh, out_, so, B, Cc, H, W, dtype)

    one = (p, 70, 2, 5, 7, COPY)
    bad = "bad arguments"
    table = (
        # a NULL pointer
        (lambda: asm(null_sources=True), INVALID, bad), (lambda: asm(hx=None), INVALID, bad),
        (lambda: asm(srcs=((None, 70, 2, 5, 7, COPY),)), INVALID, "source 0: bad arguments"),
        (lambda: reset(ar=None), INVALID, bad), (lambda: reset(cr=None), INVALID, bad), (lambda: reset(h=None), INVALID, bad),
        (lambda: reset(hx=None), INVALID, bad),
        (lambda: update(az=None), INVALID, bad), (lambda: update(cz=None), INVALID, bad), (lambda: update(aq=None), INVALID, bad),
        (lambda: update(cq=None), INVALID, bad), (lambda: update(h=None), INVALID, bad), (lambda: update(out_=None), INVALID, bad),
        # B, C, H or W <= 0
        (lambda: asm(B=0), INVALID, bad), (lambda: asm(H=0), INVALID, bad), (lambda: asm(W=-1), INVALID, bad),
        (lambda: asm(srcs=((p, 70, 0, 5, 7, COPY),)), INVALID, "source 0: bad arguments"),
        (lambda: asm(srcs=(one, (p, 70, 2, 0, 7, INTERP))), INVALID, "source 1: bad arguments"),
        (lambda: asm(srcs=(one, (p, 70, 2, 5, -7, INTERP))), INVALID, "source 1: bad arguments"),
        (lambda: reset(B=0), INVALID, bad), (lambda: reset(Cc=0), INVALID, bad), (lambda: reset(H=0), INVALID, bad),
        (lambda: reset(W=-3), INVALID, bad),
        (lambda: update(B=-1), INVALID, bad), (lambda: update(Cc=0), INVALID, bad), (lambda: update(H=0), INVALID, bad),
        (lambda: update(W=0), INVALID, bad),
        # a frame stride below C*H*W
        (lambda: asm(srcs=((p, 69, 2, 5, 7, COPY),)), INVALID, "vppx_raft_gru_assemble: source_frame_stride 69 is less than 2 planes of 5x7"),
        (lambda: asm(srcs=(one, (p, 11, 1, 3, 4, INTERP))), INVALID, "source_frame_stride 11"),
        (lambda: reset(sar=104), INVALID, "vppx_raft_gru_reset: ar_frame_stride 104 is less than 3 planes of 5x7"),
        (lambda: reset(scr=0), INVALID, "cr_frame_stride 0"), (lambda: reset(sh=-105), INVALID, "h_frame_stride -105"),
        (lambda: reset(shx=174), INVALID, "hx_frame_stride 174 is less than 5 planes"),
        (lambda: update(saz=104), INVALID, "az_frame_stride 104"), (lambda: update(scz=1), INVALID, "cz_frame_stride 1"),
        (lambda: update(saq=104), INVALID, "aq_frame_stride"), (lambda: update(scq=104), INVALID, "cq_frame_stride"),
        (lambda: update(sh=104), INVALID, "h_frame_stride"),
        (lambda: update(so=104), INVALID, "vppx_raft_gru_update: out_frame_stride 104 is less than 3 planes of 5x7"),
        # a dtype other than the two
        (lambda: asm(dtype=2), INVALID, "vppx_raft_gru_assemble: dtype 2 is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)"),
        (lambda: reset(dtype=2), INVALID, "vppx_raft_gru_reset: dtype 2"), (lambda: update(dtype=-1), INVALID, "vppx_raft_gru_update: dtype -1"),
        # more than four sources, or none
        (lambda: asm(srcs=(one,) * 5, hxc=10), INVALID, "vppx_raft_gru_assemble: 5 sources, 1 .. 4 are taken"),
        (lambda: asm(srcs=(), n=0), INVALID, "0 sources"), (lambda: asm(n=-1), INVALID, "-1 sources"),
        # an unknown mode
        (lambda: asm(srcs=((p, 70, 2, 5, 7, 3),)), INVALID, "source 0: mode 3 is not"),
        (lambda: asm(srcs=(one, (p, 70, 2, 5, 7, -1))), INVALID, "source 1: mode -1"),
        # a pool2x source of the wrong size, a copied one of another size
        (lambda: asm(srcs=((p, 300, 2, 11, 14, POOL),)), INVALID, "source 0 is 11x14 and pools to 6x7, hx is 5x7"),
        (lambda: asm(srcs=((p, 300, 2, 10, 12, POOL),)), INVALID, "pools to 5x6"),
        (lambda: asm(srcs=((p, 300, 2, 5, 7, POOL),)), INVALID, "pools to 3x4"),
        (lambda: asm(srcs=((p, 70, 2, 5, 6, COPY),)), INVALID, "source 0 is copied and is 5x6, hx is 5x7"),
        # an hx smaller than its sources' channels
        (lambda: asm(hxc=1), INVALID, "vppx_raft_gru_assemble: hx has 1 channels, the sources have 2"),
        (lambda: asm(srcs=(one, (p, 24, 2, 3, 4, INTERP)), hxc=3), INVALID, "hx has 3 channels, the sources have 4"),
        (lambda: reset(hxc=2), INVALID, "vppx_raft_gru_reset: hx has 2 channels, h has 3"),
        # more cells than one launch takes
        (lambda: asm(srcs=((p, 1 << 40, 1 << 20, 1024, 1024, COPY),), B=1 << 10, H=1024, W=1024, hxc=1 << 20), UNSUPPORTED,
         "more than one launch takes"),
        (lambda: reset(B=1 << 20, Cc=1 << 14, H=256, W=256, sar=1 << 30, scr=1 << 30, sh=1 << 30, shx=1 << 30, hxc=1 << 14), UNSUPPORTED,
         "more than one launch takes"),
        (lambda: update(B=1 << 20, Cc=1 << 14, H=256, W=256, saz=1 << 30, scz=1 << 30, saq=1 << 30, scq=1 << 30, sh=1 << 30, so=1 << 30),
         UNSUPPORTED, "more than one launch takes"),
        (lambda: update(H=1 << 16, W=1 << 16, saz=1 << 40, scz=1 << 40, saq=1 << 40, scq=1 << 40, sh=1 << 40, so=1 << 40), UNSUPPORTED,
         "map is more than the call takes"),
    )
    for n, (call, code, msg) in enumerate(table):
        rc = call()
        text = lib.vppx_last_error().decode()
        assert rc == code and msg in text, (n, rc, code, msg, text)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL32).all() and (inp.cpu().numpy() == 1.0).all()
    # what is allowed: the smallest of everything
    assert asm(srcs=((p, 1, 1, 1, 1, COPY), (p, 1, 1, 1, 1, POOL), (p, 1, 1, 1, 1, INTERP)), H=1, W=1, hxc=3) == 0
    assert reset(B=1, Cc=1, H=1, W=1, sar=1, scr=1, sh=1, shx=1, hxc=1) == 0
    assert update(B=1, Cc=1, H=1, W=1, saz=1, scz=1, saq=1, scq=1, sh=1, so=1) == 0
    torch.cuda.synchronize()
    assert (inp.cpu().numpy() == 1.0).all() and (out.cpu().numpy()[3:] == SENTINEL32).all()

    # through Engine
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=eng.device)            # noqa: E731
    with pytest.raises(ValueError, match="unknown mode"):
        eng.raft_gru_assemble([(f32(1, 2, 5, 7), "pool4x")])
    with pytest.raises(ValueError, match="5 given"):
        eng.raft_gru_assemble([(f32(1, 2, 5, 7), "copy")] * 5)
    with pytest.raises(ValueError, match="no copied source"):
        eng.raft_gru_assemble([(f32(1, 2, 5, 7), "interp")])
    with pytest.raises(ValueError, match=r"sources\[1\]: expected a torch.float32"):
        eng.raft_gru_assemble([(f32(1, 2, 5, 7), "copy"), (f32(1, 2, 5, 7).bfloat16(), "copy")])
    with pytest.raises(ValueError, match="every frame must be contiguous"):
        eng.raft_gru_assemble([(f32(1, 2, 5, 14)[..., ::2], "copy")])
    with pytest.raises(ValueError, match=r"sources\[1\]: 2 frames"):
        eng.raft_gru_assemble([(f32(1, 2, 5, 7), "copy"), (f32(2, 2, 5, 7), "copy")])
    with pytest.raises(_lib.VppxError) as e:
        eng.raft_gru_assemble([(f32(1, 2, 5, 7), "copy"), (f32(1, 2, 11, 14), "pool2x")])
    assert e.value.code == INVALID
    with pytest.raises(ValueError, match="ar: expected shape"):
        eng.raft_gru_reset(f32(1, 3, 5, 7), f32(1, 2, 5, 7), f32(1, 2, 5, 7), f32(1, 4, 5, 7))
    with pytest.raises(ValueError, match="hx: expected"):
        eng.raft_gru_reset(f32(1, 2, 5, 7), f32(1, 2, 5, 7), f32(1, 2, 5, 7), f32(1, 4, 5, 6))
    with pytest.raises(_lib.VppxError):
        eng.raft_gru_reset(f32(1, 2, 5, 7), f32(1, 2, 5, 7), f32(1, 2, 5, 7), f32(1, 1, 5, 7))
    with pytest.raises(ValueError, match="cq: expected a torch.float32"):
        eng.raft_gru_update(f32(1, 2, 5, 7), f32(1, 2, 5, 7), f32(1, 2, 5, 7), f32(1, 2, 5, 7).half(), f32(1, 2, 5, 7))
    with pytest.raises(ValueError, match="out: expected shape"):
        eng.raft_gru_update(*([f32(1, 2, 5, 7)] * 5), out=f32(1, 2, 5, 8))


# ---- FusedUpdate ---------------------------------------------------------------------------------------------------------
ORDER = ["gru32.convz", "gru32.convr", "gru32.convq", "gru16.convz", "gru16.convr", "gru16.convq", "convc1", "convc2", "convf1", "convf2",
         "conv", "gru08.convz", "gru08.convr", "gru08.convq", "flow_head", "mask"]


def _ref_key(name):
    if name in R.ENCODER_CONVS:
        return name
    if name in ("flow_head", "mask"):
        return "net0"
    return name.split(".")[0] + (".rhx" if name.endswith("convq") else ".hx")


class _Replay:
    """A stand-in BasicMultiUpdateBlock whose "convolutions" replay one recorded call: each holds its input to the
    referee's limit around what the reference's convolution was given, then returns what that convolution returned."""

    def __init__(self, eng, G):
        self.eng, self.G, self.n_gru_layers = eng, G, 3
        self.encoder = SimpleNamespace(**{n: self._conv(n) for n in R.ENCODER_CONVS})
        for lvl in ("gru08", "gru16", "gru32"):
            setattr(self, lvl, SimpleNamespace(**{cv: self._conv(f"{lvl}.{cv}") for cv in ("convz", "convr", "convq")}))
        self.flow_head, self.mask = self._conv("flow_head"), self._conv("mask")

    def arm(self, call):
        self.call, self.refs, self.seen = call, R.block_ref(self.G, call, DEVICE_EXP_ULPS), []

    def _conv(self, name):
        def conv(x):
            import torch
            assert x.dtype == torch.float32 and x.is_contiguous()
            hold(R, _host(x), self.refs[_ref_key(name)], f"{self.call}: the input of {name}")
            self.seen.append(name)
            return _dev(self.eng, self.G[f"{self.call}_{name}_out"])
        return conv


def test_fused_update_replays_the_recording(eng):
    import torch
    from vppstereo_amd.update import FusedUpdate
    G = R.load_recording()
    blk = _Replay(eng, G)
    fused = FusedUpdate(blk)
    assert fused.n_gru_layers == 3 and fused.gru08 is blk.gru08
    buffers = {}
    for call in R.CALLS:
        blk.arm(call)
        flags = R.CALL_FLAGS[call]
        net = [_dev(eng, G[f"{call}_net{i}_in"]) for i in range(3)]
        net_in = list(net)
        inp = [list(_dev(eng, G[f"{call}_inp{i}"]).split(G[f"{call}_net{i}_in"].shape[1], dim=1)) for i in range(3)]
        corr = _dev(eng, G[f"{call}_corr"]) if flags["iter08"] else None
        flow = _dev(eng, G[f"{call}_flow"]) if flags["iter08"] else None
        res = fused(net, inp, corr, flow, **flags)
        torch.cuda.synchronize()
        want = [n for n in ORDER if (n.startswith("gru32") and flags["iter32"]) or (n.startswith("gru16") and flags["iter16"]) or
                (flags["iter08"] and not n.startswith(("gru32", "gru16", "flow_head", "mask"))) or (flags["update"] and n in ("flow_head", "mask"))]
        assert blk.seen == want, (call, blk.seen)
        if flags["update"]:
            net_out, mask, delta = res
            assert np.array_equal(_host(mask), G[f"{call}_mask"]) and np.array_equal(_host(delta), G[f"{call}_delta"])
        else:
            net_out = res
        assert net_out is net
        for i in range(3):
            if f"net{i}" in blk.refs:
                ref = blk.refs[f"net{i}"]
                got = _host(net_out[i])
                hold(R, got, ref, f"{call}: net[{i}]")
                assert (np.abs(got.astype(F64) - G[f"{call}_net{i}_out"]) <= 2 * ref.limit).all()   # both lie within the limit of one value
                assert net_out[i].data_ptr() != net_in[i].data_ptr()
            else:
                assert net_out[i] is net_in[i]
        for level, buf in fused._hx.items():           # one hx buffer per level, kept from call to call
            assert buffers.setdefault(level, buf.data_ptr()) == buf.data_ptr()
    assert sorted(buffers) == [8, 16, 32]


def _live_block(n_gru_layers, hid, log):
    """A block whose "convolutions" are pointwise torch expressions (no convolution library): Cout channels from the sum
    over the input's channels.  Each keeps what it was given and what it returned."""
    import torch

    def conv(name, cout):
        def f(x):
            s = x.float().sum(dim=1, keepdim=True)
            k = torch.linspace(-1.5, 1.5, cout, device=x.device).view(1, cout, 1, 1)
            y = (torch.sin(s * 0.7 + k) * 4.0 * (1 + k)).to(x.dtype)
            log.append((name, x.clone(), y))
            return y
        return f

    blk = SimpleNamespace(n_gru_layers=n_gru_layers)
    blk.encoder = SimpleNamespace(convc1=conv("convc1", 5), convc2=conv("convc2", 5), convf1=conv("convf1", 4), convf2=conv("convf2", 4),
                                  conv=conv("conv", 6))
    for lvl in ("gru08", "gru16", "gru32"):
        setattr(blk, lvl, SimpleNamespace(**{cv: conv(f"{lvl}.{cv}", hid) for cv in ("convz", "convr", "convq")}))
    blk.flow_head, blk.mask = conv("flow_head", 2), conv("mask", 9)
    return blk


@pytest.mark.parametrize("n_gru_layers", [3, 2, 1])
def test_fused_update_through_changing_shapes(eng, n_gru_layers):
    """One FusedUpdate object, called with another B, another shape and the other dtype in turn, and back: every
    convolution's input is held to the referee around the tensors the call itself produced."""
    import torch
    from vppstereo_amd.update import FusedUpdate
    hid, log = 4, []
    fused = FusedUpdate(_live_block(n_gru_layers, hid, log))
    rng = np.random.default_rng([4403, n_gru_layers])
    plan = [(1, (5, 6), "float32"), (2, (7, 9), "float32"), (2, (7, 9), "bfloat16"), (1, (8, 16), "bfloat16"), (1, (5, 6), "float32")]
    for step, (B, s0, dtype) in enumerate(plan):
        sizes = [s0]
        for _ in range(2):
            sizes.append(tuple(R.pooled_size(v) for v in sizes[-1]))
        mk = lambda *shape, scale=1.0: (rng.standard_normal(shape) * scale).astype(F32) if dtype == "float32" else R.to_bf16(  # noqa: E731
            (rng.standard_normal(shape) * scale).astype(F32))
        net_h = [np.tanh(mk(B, hid, *s)).astype(F32) for s in sizes]
        if dtype == "bfloat16":
            net_h = [R.to_bf16(a) for a in net_h]
        inp_h = [mk(B, 3 * hid, *s, scale=2.0) for s in sizes]
        corr_h, flow_h = mk(B, 3, *s0), mk(B, 2, *s0, scale=3.0)
        net = [_dev(eng, a, dtype) for a in net_h]
        inp = [list(_dev(eng, a, dtype).split(hid, dim=1)) for a in inp_h]
        del log[:]
        flags = dict(iter32=n_gru_layers == 3, iter16=n_gru_layers >= 2)
        net_out, mask, delta = fused(net, inp, _dev(eng, corr_h, dtype), _dev(eng, flow_h, dtype), **flags)
        torch.cuda.synchronize()
        seen = {name: (_host(x), _host(y)) for name, x, y in log}
        assert [name for name, _, _ in log] == [n for n in ORDER if (flags["iter32"] or not n.startswith("gru32")) and
                                                (flags["iter16"] or not n.startswith("gru16"))]
        new = [_host(t) for t in net_out]
        relu = lambda a: np.maximum(a, 0)                                                 # noqa: E731
        levels = []
        if flags["iter32"]:
            levels.append(("gru32", 2, [(net_h[1], "pool2x")]))
        if flags["iter16"]:
            levels.append(("gru16", 1, [(net_h[0], "pool2x")] + ([(new[2], "interp")] if n_gru_layers > 2 else [])))
        levels.append(("gru08", 0, [(relu(seen["conv"][1]), "copy"), (flow_h, "copy")] + ([(new[1], "interp")] if n_gru_layers > 1 else [])))
        for tag, i, sources in levels:
            cz, cr, cq = np.split(inp_h[i], 3, axis=1)
            hx, rhx, h_new = R.gru_ref(net_h[i], sources, cz, cr, cq, seen[f"{tag}.convz"][1], seen[f"{tag}.convr"][1], seen[f"{tag}.convq"][1],
                                       DEVICE_EXP_ULPS)
            what = f"step {step} {tag}"
            hold(R, seen[f"{tag}.convz"][0], hx, f"{what}: hx", dtype)
            assert np.array_equal(seen[f"{tag}.convr"][0], seen[f"{tag}.convz"][0])
            hold(R, seen[f"{tag}.convq"][0], rhx, f"{what}: [r*h, x]", dtype)
            hold(R, new[i], h_new, f"{what}: the new state", dtype)
        assert np.array_equal(seen["flow_head"][0], new[0]) and np.array_equal(seen["mask"][0], new[0])
        assert np.array_equal(_host(delta), seen["flow_head"][1])
        assert np.array_equal(_host(mask), _host((0.25 * _dev(eng, seen["mask"][1], dtype))))
        for i in range(3):
            if not any(i == j for _, j, _ in levels):
                assert net_out[i] is net[i] or np.array_equal(new[i], net_h[i])
        for level, buf in fused._hx.items():
            assert buf.shape[0] == B and buf.dtype == _tdtype(dtype) and tuple(buf.shape[2:]) == sizes[{8: 0, 16: 1, 32: 2}[level]]


def test_fused_gru_alone(eng):
    from vppstereo_amd.update import fused_gru
    c, _, ref_u = _gate_ref("c3_5x7", "float32")
    log = []
    gru = SimpleNamespace(convz=lambda hx: log.append(_host(hx)) or _dev(eng, c.az), convr=lambda hx: _dev(eng, c.ar),
                          convq=lambda hx: log.append(_host(hx)) or _dev(eng, c.aq))
    cz, cr, cq = _dev(eng, c.c).split(c.C, dim=1)
    h, x = _dev(eng, c.h), _dev(eng, c.x)
    got = fused_gru(gru, h, cz, cr, cq, x)
    hold(R, _host(got), ref_u, "fused_gru")
    assert np.array_equal(log[0].view(np.uint32), np.concatenate([c.h, c.x], axis=1).view(np.uint32))
    hold(R, log[1][:, :c.C], R.reset(c.ar, c.cr, c.h, DEVICE_EXP_ULPS), "fused_gru: r*h")
    assert np.array_equal(log[1][:, c.C:], c.x)
