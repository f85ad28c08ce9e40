"""GPU: the device PNG decoder (csrc/png_kernels.hip) on DEFLATE streams written construct by construct.

tests/test_gpu_png.py feeds the decoder what zlib's and PIL's encoders happen to emit.  Here every Huffman code length, match
length, distance, block boundary and code-length run is chosen: tests/_png_streams.py builds the files with the writer of
tests/_deflate.py, tests/test_deflate_cpu.py holds them to zlib and PIL and asserts -- without a GPU -- that each file holds the
constructs it is named for.  Valid files must decode to the scalar reference unfilter of their inflated bytes, bit for bit;
malformed ones must get the status include/vppx.h documents, and must not disturb their neighbours in a batch.

Every refusal is a documented status, not a fault: each case names, in `Refusal.why`, the check in png_kernels.hip that ends
it (shown when the case fails), and none of them reads or writes outside the masked ring, the zero-padded input window or the
code-length array, whatever the input.
"""
import ctypes as C

import numpy as np
import pytest

import _deflate as D
import _png_streams as S

pytestmark = pytest.mark.gpu

SENT_F, SENT_V, SENT_U = -7.0, 0xAB, 0xCD


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _decode(eng, files, H, W, channels=1, want="disp", scale=1.0):
    """vppx_png_decode_dev with the per-file status: (status, disp, valid) or (status, u8); the outputs start out filled with
    sentinels, so an untouched file shows"""
    from vppstereo_amd import _lib
    from vppstereo_amd.engine import _ptr
    torch = eng.torch
    n = len(files)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(b) for b in files])
    blob = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).to(eng.device)
    status = torch.full((n,), -1, dtype=torch.int32, device=eng.device)
    disp = valid = out = None
    if want == "disp":
        disp = torch.full((n, H, W), SENT_F, dtype=torch.float32, device=eng.device)
        valid = torch.full((n, H, W), SENT_V, dtype=torch.uint8, device=eng.device)
    else:
        out = torch.full((n, H, W, channels), SENT_U, dtype=torch.uint8, device=eng.device)
    eng._bind_stream()
    _lib.check(eng.lib.vppx_png_decode_dev(eng.ctx.handle, n, _ptr(blob), offs.ctypes.data_as(C.POINTER(C.c_int64)), int(H), int(W),
                                           int(channels), float(scale), _ptr(disp), _ptr(valid), _ptr(out), _ptr(status)))
    st = status.cpu().numpy()
    if want == "disp":
        return st, disp.cpu().numpy(), valid.cpu().numpy()
    return st, out.cpu().numpy()


def _check_exact(eng, files, expect, H, W, depth, channels):
    """disp / valid (gray) and the 8-bit output (8-bit files) of a batch of files that all decode to `expect[i]`"""
    if channels == 1:
        disp, valid = eng.png_decode(files, H, W)
        disp, valid = disp.cpu().numpy(), valid.cpu().numpy()
        for i, e in enumerate(expect):
            ref = e / 256.0                                             # exact in float32: samples have 16 bits
            assert np.array_equal(disp[i].astype(np.float64), ref), i
            assert np.array_equal(valid[i], (e > 0).astype(np.uint8)), i
    if depth == 8:
        out = eng.png_decode(files, H, W, channels=channels, want="u8").cpu().numpy()
        for i, e in enumerate(expect):
            assert np.array_equal(out[i], e.reshape(H, W, channels)), i


# ----------------------------------------------------------------------------------------------------------- valid streams
@pytest.mark.parametrize("build", S.VALID, ids=lambda f: f.__name__)
def test_hand_built_streams_decode_to_the_reference_unfilter(eng, build):
    """long codes (15 bits deep in both alphabets, every length and distance symbol), the same tokens through a fixed block,
    self-overlapping matches, the block sequence with matches reaching back across block boundaries into stored blocks,
    stored blocks at every bit offset, the dynamic-header seams: what each holds is asserted in tests/test_deflate_cpu.py.
    (16-bit files have no 8-bit output: that request is refused, row 15 of the table.)"""
    c = build()
    _check_exact(eng, [c.png], [c.expect], c.H, c.W, c.depth, c.channels)
    st, disp, valid = _decode(eng, [c.png], c.H, c.W, scale=1.0)        # readDispMidd's scale, and the status itself
    assert st.tolist() == [0]
    assert np.array_equal(disp[0], c.expect.astype(np.float32)) and np.array_equal(valid[0], (c.expect > 0).astype(np.uint8))


# ------------------------------------------------------------------------------------------------- geometry and filters
GEOM_W = (1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65)


def _picture(rng, kind, H, W):
    if kind == "gray16":
        return rng.integers(0, 65536, (H, W)).astype(np.uint16)
    return rng.integers(0, 256, (H, W) if kind == "gray8" else (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("H", (1, 6))
@pytest.mark.parametrize("kind", ("gray8", "gray16", "rgb8"))
def test_every_filter_on_every_row_at_narrow_widths(eng, kind, H):
    """bytes per pixel 1, 2, 3 at W = 1..9 (the tails of the serial Average / Paeth loop, unrolled by 4 pixels) and 63, 64, 65
    (the Sub scan with fewer pixels than lanes, with exactly as many, with one more); each of the five filter types on row 0
    and on every later row (the five rotations), zlib levels 0 (stored) and 6."""
    rng = np.random.default_rng(H)
    depth, channels = (16 if kind == "gray16" else 8), (3 if kind == "rgb8" else 1)
    for W in GEOM_W:
        files, expect = [], []
        for rot in range(5):
            types = tuple((rot + k) % 5 for k in range(5))
            for level in (0, 6):
                a = _picture(rng, kind, H, W)
                files.append(D._raw_png(a, types=types, level=level, extra=False))
                expect.append(a)
        _check_exact(eng, files, expect, H, W, depth, channels)


def test_paeth_ties_and_average_carry(eng):
    """Paeth where the predictor hangs on a tie (pa == pb picks the left byte, pb == pc the byte above; all three equal), counted
    on the reference; Average where left + above does not fit 8 bits."""
    rng = np.random.default_rng(11)
    a, ties = S.paeth_tie_picture()                                     # (built and counted without a GPU, too)
    H, W = a.shape
    assert min(ties[k] for k in ("pa==pb", "pb==pc", "all")) >= 1, ties
    _check_exact(eng, [D._raw_png(a, types=(4,), level=lvl, extra=False) for lvl in (0, 6)], [a, a], H, W, 8, 1)
    a16 = (rng.integers(0, 4, (H, W)) * 0x0A0A + 0x3C3C).astype(np.uint16)
    _check_exact(eng, [D._raw_png(a16, types=(4,), extra=False)], [a16], H, W, 16, 1)
    b = rng.integers(200, 256, (H, W), dtype=np.uint8)
    assert (b[1:, :-1].astype(int) + b[:-1, 1:] > 255).all()
    _check_exact(eng, [D._raw_png(b, types=(3,), level=lvl, extra=False) for lvl in (0, 6)], [b, b], H, W, 8, 1)
    rgb = rng.integers(200, 256, (H, W, 3), dtype=np.uint8)
    _check_exact(eng, [D._raw_png(rgb, types=(3, 4), extra=False)], [rgb], H, W, 8, 3)


def test_widest_scanline_wraps_the_ring(eng):
    """16-bit gray W = 8191: scanlines of 16383 bytes, the most the decoder takes; with H = 5 the fifth row wraps the 64 KB
    window.  All five filters, random samples (zlib stores or Huffman-codes them), levels 0 and 6."""
    rng = np.random.default_rng(12)
    a = rng.integers(0, 65536, (5, 8191)).astype(np.uint16)
    files = [D._raw_png(a, level=lvl, extra=False) for lvl in (0, 6)]
    _check_exact(eng, files, [a, a], 5, 8191, 16, 1)


def test_adler_sums_of_the_widest_all_ones_rows(eng):
    """the same width, six rows, every sample 0xFFFF behind filter type 0: every filtered byte is 0xFF, the largest the
    per-lane and per-wave partial sums of the Adler-32 get (png_row's overflow comment); a wrong sum is status 9"""
    a = np.full((6, 8191), 0xFFFF, np.uint16)
    files = [D._raw_png(a, types=(0,), level=lvl, extra=False) for lvl in (0, 6)]
    _check_exact(eng, files, [a, a], 6, 8191, 16, 1)
    st, _, _ = _decode(eng, files, 6, 8191)
    assert st.tolist() == [0, 0]


def test_widest_rgb_row_and_the_api_limit(eng):
    rng = np.random.default_rng(13)
    a = rng.integers(0, 256, (4, 2730, 3), dtype=np.uint8)
    a[2] = a[1]
    _check_exact(eng, [D._raw_png(a, extra=False)], [a], 4, 2730, 8, 3)
    g = rng.integers(0, 256, (2, 8192), dtype=np.uint8)
    with pytest.raises(Exception, match="scanlines longer than 16 KB"):
        eng.png_decode([D._raw_png(g, extra=False)], 2, 8192, channels=1, want="u8")


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("r", S.refusals(), ids=lambda r: r.id)
def test_refusals_get_their_documented_status(eng, r):
    """rows 1..18 of the table in DESIGN.md section 7 / include/vppx.h; r.why names the check that ends the case"""
    got = _decode(eng, [r.png], r.H, r.W, r.channels, r.want)
    assert got[0].tolist() == [r.status], (r.id, r.why, got[0])
    rowb, done = 1 + r.W * r.channels, r.rows                           # (files that get as far as a scanline are 8-bit gray)
    for o, sent in zip(got[1:], (SENT_F, SENT_V) if r.want == "disp" else (SENT_U,)):
        assert (o[0, done:] == np.asarray(sent, o.dtype)).all(), (r.id, "rows past the failure were written")
    if done:
        want = D.unfilter(r.raw[:done * rowb], done, rowb, 1)
        assert np.array_equal(got[1][0, :done], want.astype(np.float32))


def test_engine_raises_with_the_status(eng):
    r = S.refusal("one-distance-code-of-length-2")
    with pytest.raises(ValueError, match="status 6"):
        eng.png_decode([S.small_good(1)[0], r.png], r.H, r.W)
    r = S.refusal("gray16-into-u8")
    with pytest.raises(ValueError, match="file 0 rejected with status 3"):
        eng.png_decode([r.png], r.H, r.W, channels=1, want="u8")


def test_a_refused_file_leaves_its_neighbours_alone(eng):
    """one call: [good, over-subscribed lengths, good, filter byte 5 on the last row, good]"""
    goods = [S.small_good(k) for k in (1, 2, 3)]
    assert len({g[0] for g in goods}) == 3
    r1, r17 = S.refusal("litlen-oversubscribed"), S.refusal("filter-5-on-row-2")
    files = [goods[0][0], r1.png, goods[1][0], r17.png, goods[2][0]]
    for want in ("disp", "u8"):
        got = _decode(eng, files, S.RH, S.RW, 1, want)
        assert got[0].tolist() == [0, 6, 0, 7, 0]
        o = got[1]
        for k, i in enumerate((0, 2, 4)):
            assert np.array_equal(o[i].reshape(S.RH, S.RW), goods[k][1].astype(o.dtype))
        sent = SENT_F if want == "disp" else SENT_U
        assert (o[1] == np.asarray(sent, o.dtype)).all()                # failed before its first scanline: untouched
        rows = D.unfilter(r17.raw[:2 * (1 + S.RW)], 2, 1 + S.RW, 1)
        assert np.array_equal(o[3].reshape(S.RH, S.RW)[:2], rows.astype(o.dtype))     # the scanlines decoded so far
        assert (o[3].reshape(S.RH, S.RW)[2] == np.asarray(sent, o.dtype)).all()
        if want == "disp":
            assert (got[2][1] == SENT_V).all() and (got[2][3][2] == SENT_V).all()
            assert np.array_equal(got[2][3][:2], (rows > 0).astype(np.uint8))
