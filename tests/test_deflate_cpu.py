"""No GPU: the DEFLATE writer of tests/_deflate.py and the files tests/_png_streams.py builds with it, held to zlib and PIL,
and the coverage claims of tests/test_gpu_png_streams.py asserted from what the writer recorded while it wrote.

A stream that misses the construct it was written for tests nothing and says nothing: here every claim ("a 15-bit distance code
was decoded", "a stored block began at bit 5") is an assertion on the stream's record, so a change to a generator that loses a
construct fails here, without a GPU."""
import functools
import io
import zlib

import numpy as np
import pytest

import _deflate as D
import _png_streams as S


def _pil(png):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(png)))


# -------------------------------------------------------------------------------------------------------------- the writer
def test_bit_writer_orders():
    w = D.BitWriter()
    w.bits(0b101, 3)            # fields: LSB first
    w.code(0b110, 3)            # codes: MSB first -> 0, 1, 1 into bits 3, 4, 5
    w.bits(1, 1)
    assert w.bitpos == 7 and w.getvalue() == bytes([0b1011101 | 0])
    w.align()
    w.raw(b"\xAB")
    assert w.getvalue() == bytes([0b01011101, 0xAB]) and w.bitpos == 16


def test_canonical_codes_are_rfc1951s_example():
    # RFC 1951 3.2.2: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> codes 010 011 100 101 110 00 1110 1111
    assert D.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [0b010, 0b011, 0b100, 0b101, 0b110, 0b00, 0b1110, 0b1111]
    assert D.canonical(D.FIXED_LLENS)[0] == 0b00110000 and D.canonical(D.FIXED_LLENS)[144] == 0b110010000
    assert D.canonical(D.FIXED_LLENS)[256] == 0 and D.canonical(D.FIXED_LLENS)[280] == 0b11000000


@pytest.mark.parametrize("n,depth,split", [(35, 15, 9), (30, 15, 8), (16, 15, None), (2, 1, None), (9, 6, None), (256, 8, None)])
def test_complete_lengths(n, depth, split):
    lens = D.complete_lengths(n, depth, split)
    assert len(lens) == n and D.kraft(lens) == 1 << 15 and max(lens) == depth
    if split is not None:                                   # every length the long-code walk can end at stays populated
        assert set(range(split + 1, depth + 1)) <= set(lens) and set(range(1, split)) <= set(lens)


def test_symbols_of_lengths_and_distances():
    for length in range(3, 259):
        s, nb, v = D.length_symbol(length)
        assert D.LEN_BASE[s - 257] + v == length and v < (1 << nb) and nb == D.LEN_EXTRA[s - 257]
    assert D.length_symbol(258) == (285, 0, 0) and D.length_symbol(258, True) == (284, 5, 31) and D.length_symbol(257) == (284, 5, 30)
    for dist in (1, 2, 3, 4, 5, 6, 7, 24576, 24577, 32767, 32768):
        s, nb, v = D.dist_symbol(dist)
        assert D.DIST_BASE[s] + v == dist and v < (1 << nb)
    assert D.dist_symbol(32768) == (29, 13, 8191) and D.dist_symbol(16385) == (28, 13, 0)


def test_reference_expansion():
    assert D.reference([1, 2, 3, (5, 3)]) == bytes([1, 2, 3, 1, 2, 3, 1, 2])
    assert D.reference([(4, 1)], b"\x07") == b"\x07" * 4
    assert D.reference([9, (3, 2)], b"\x01\x02") == bytes([9, 2, 9, 2])


def test_code_length_sequences():
    lens = [0] * 150 + [3] * 9 + [0, 0, 4] + [0] * 5
    for seq in (D.plain(lens), D.rle(lens)):
        assert D.expand_cl_seq(seq)[0] == lens
    assert D.expand_cl_seq([5, (16, 3), (17, 4), (16, 3)]) == ([5] * 4 + [0] * 7, [(16, 1, 3, 5), (17, 4, 4, 16), (16, 8, 3, 17)])


def test_stored_blocks_of_0_and_65535_bytes_and_every_block_kind_inflate():
    rng = np.random.default_rng(0)
    big = bytes(rng.integers(0, 256, 65535, dtype=np.uint8))
    s = D.Deflate()
    s.stored(b"")
    s.stored(big)
    s.fixed([200, 0, (258, 1, True), (3, 32768)])
    ll = D.spread_lengths({7, 256, 285}, 286, 2, rng)
    s.dynamic([7, (258, 32768)], ll, [0] * 29 + [1], cl_seq=D.rle(ll + [0] * 29 + [1]))
    s.stored(b"", final=True)
    raw = bytes(s.out)
    assert len(raw) == 65535 + 2 + 258 + 3 + 1 + 258
    assert zlib.decompress(D.zlib_wrap(s.getvalue(), raw)) == raw
    assert zlib.decompress(s.getvalue(), wbits=-15) == raw


def test_unfilter_inverts_filter_rows():
    rng = np.random.default_rng(1)
    for bpp, W in ((1, 9), (2, 5), (3, 4)):
        rows = rng.integers(0, 256, (7, W * bpp), dtype=np.uint8)
        raw = D._filter_rows(rows, bpp, (4, 3, 2, 1, 0))
        assert np.array_equal(D.unfilter(raw, 7, 1 + W * bpp, bpp), rows)


# ----------------------------------------------------------------------------------------------------------- valid streams
def _small_good(seed):
    f = functools.partial(S.small_good_case, seed)
    f.__name__ = "small_good_%d" % seed
    return f


SMALL_GOOD = [_small_good(k) for k in (1, 2, 3)]                       # the batch test's good neighbours


@pytest.mark.parametrize("build", list(S.VALID) + SMALL_GOOD, ids=lambda f: f.__name__)
def test_zlib_and_pil_agree_with_the_reference(build):
    c = build()
    assert zlib.decompress(c.z) == c.raw
    assert len(c.png) < 110_000
    got = _pil(c.png)
    assert got.shape == c.expect.shape and np.array_equal(got.astype(np.int64), c.expect.astype(np.int64))


def test_long_codes_claims():
    c = S.long_codes()
    f = c.feat
    assert len(f["runs"]) == 1                                          # one dynamic block
    assert set(range(11, 16)) <= f["lit_code_lens"]["dynamic"] and 10 in f["lit_code_lens"]["dynamic"]  # walk (> 10 bits) and table edge
    assert set(range(10, 16)) <= f["dist_code_lens"]["dynamic"] and 9 in f["dist_code_lens"]["dynamic"]
    assert min(f["lit_code_lens"]["dynamic"]) <= 3 and min(f["dist_code_lens"]["dynamic"]) <= 3
    assert f["dist_syms"] == set(range(30)) and f["len_syms"] == set(range(257, 286))
    for s in range(30):
        assert {0, (1 << D.DIST_EXTRA[s]) - 1} <= f["dist_extra"][s], s
    for s in range(257, 286):
        assert {0, (1 << D.LEN_EXTRA[s - 257]) - 1} <= f["len_extra"][s], s
    assert {1, 2, 3, 32767, 32768, 16385, 24576, 24577} <= f["distances"]
    assert {3, 257, 258} <= f["lengths"] and 31 in f["len_extra"][284] and 30 in f["len_extra"][284] and 285 in f["len_syms"]
    assert {1, 2} <= c.straddles() and max(c.straddles()) >= 7          # 258 bytes over scanlines of 35
    assert f["literals"] == set(range(5))


def test_fixed_same_claims():
    c = S.fixed_same()
    f = c.feat
    assert [k for k, _, _ in c.blocks] == ["fixed"]
    assert f["dist_syms"] == set(range(30)) and f["len_syms"] == set(range(257, 286))
    assert {1, 2, 3, 32767, 32768} <= f["distances"] and 31 in f["len_extra"][284]
    assert f["lit_code_lens"]["fixed"] == {7, 8, 9} and f["dist_code_lens"]["fixed"] == {5} and not f["runs"]
    assert any(b >= 144 for b in f["literals"]) and any(b < 144 for b in f["literals"])
    assert set(range(280, 286)) <= f["len_syms"]
    assert c.rowb == 16383


def test_overlap_claims():
    f = S.overlap().feat
    for d in S.OVERLAP_DISTS:
        for l in S.OVERLAP_LENS:
            assert (d, l) in f["pairs"], (d, l)
    for l in S.OVERLAP_LENS:
        assert (l, l) in f["pairs"] and (l + 1, l) in f["pairs"]
    assert {1, 2, 3, 63, 64, 65, 257} <= f["periods"] and (1, 258) in f["pairs"] and (2, 258) in f["pairs"] and (3, 258) in f["pairs"]


def test_block_sequence_claims():
    c = S.block_sequence()
    f = c.feat
    kinds = [k for k, _, _ in c.blocks]
    ends = [start for _, start, _ in c.blocks[1:]] + [len(c.raw)]
    sizes = [e - start for (k, start, _), e in zip(c.blocks, ends) if k == "stored"]
    assert kinds == ["stored", "dynamic", "stored", "stored", "fixed", "stored", "dynamic"] and sizes == [0, 1000, 0, 65535]
    assert {("fixed", "stored"), ("fixed", "dynamic"), ("dynamic", "stored")} <= f["cross"]
    assert 32768 in f["distances"]


def test_stored_offsets_claims():
    c = S.stored_offsets()
    assert c.feat["stored_bit_offsets"] == set(range(8))
    assert ("fixed", "stored") in c.feat["cross"]


def test_header_seams_claims():
    f = S.header_seams().feat
    runs = f["runs"]
    crossing = {(sym) for nlen, ndist, rr in runs for sym, idx, n, before in rr if idx < nlen < idx + n}
    assert {16, 18} <= crossing                                         # a run from the literal/length lengths into the distance lengths
    nl, nd, rr = runs[0]
    assert (nl, nd) == (286, 30) and (18, 261, 30, rr[-1][3]) == rr[-1]
    after = {(sym, before) for _, _, rr in runs for sym, idx, n, before in rr}
    assert (16, 17) in after and (16, 18) in after                      # 16 right after a run: repeats its 0
    assert any(sym == 16 and n == 6 and before not in (0, 16, 17, 18) for _, _, rr in runs for sym, idx, n, before in rr)
    assert (257, 1) in {(a, b) for a, b, _ in runs} and 257 in f["nlen"] and 286 in f["nlen"] and 30 in f["ndist"]
    assert f["hclen"] >= {5, 19}
    dl = [d for _, d in f["codes"]]
    assert (1,) in dl and (0, 0, 0, 0, 1) in dl and 4 in f["dist_syms"] and 0 in f["dist_syms"]    # one distance code, of one bit
    assert (0,) in dl                                                   # no distance code
    assert any(sum(1 for l in ll if l) == 1 and ll[256] == 1 for ll, _ in f["codes"])             # only the end-of-block code


def test_paeth_tie_picture_has_every_tie():
    _, ties = S.paeth_tie_picture()
    assert min(ties[k] for k in ("pa==pb", "pb==pc", "all")) >= 1, ties


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("r", S.refusals(), ids=lambda r: r.id)
def test_zlib_refuses_what_rows_1_to_14_hold_and_inflates_rows_15_to_18(r):
    if r.zmsg is None:
        zlib.decompress(r.z)                                            # a valid stream: the PNG layer refuses
        return
    assert r.row <= 14
    with pytest.raises(zlib.error) as e:
        zlib.decompress(r.z)
    assert r.zmsg in str(e.value), str(e.value)                         # refused for THIS reason, not as truncated
    assert r.why


def test_refusal_table_is_complete():
    rows = {r.row for r in S.refusals()}
    assert rows == set(range(1, 19))
    status = {}
    for r in S.refusals():
        status.setdefault(r.row, set()).add(r.status)
    want = {**{k: {6} for k in range(1, 11)}, **{k: {5} for k in range(11, 15)}, 15: {3}, 16: {4}, 17: {7}, 18: {3}}
    assert status == want
    assert len({r.id for r in S.refusals()}) == len(S.refusals())
