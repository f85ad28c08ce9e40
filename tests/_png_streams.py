"""The hand-built PNG files of tests/test_gpu_png_streams.py: DEFLATE streams written construct by construct with
tests/_deflate.py, valid ones with the samples they must decode to, malformed ones with the status include/vppx.h documents.

Every case is built once per process (lru_cache).  tests/test_deflate_cpu.py holds each valid case to zlib and PIL and asserts,
from what the writer recorded, that the case holds the constructs it was written for; it holds each malformed stream to zlib's
refusal.  The GPU test then only has to compare bytes.

Literals of the Huffman-coded cases come from {0..4} unless a case says otherwise: every byte is then a legal PNG filter type,
so a match may start, end and land anywhere in the scanline grid.
"""
import functools
import struct
import zlib

import numpy as np

import _deflate as D


class Gen:
    """A token generator that keeps the inflated stream legal as PNG scanlines of `rowb` bytes.  lit_any = False: all bytes
    are 0..4.  lit_any = True: bytes off the row starts are arbitrary (half of them >= 144, the 9-bit fixed codes), and a match
    that would copy an illegal byte onto a row start is preceded by filler up to that row start and a literal filter byte."""

    def __init__(self, rng, rowb, lit_any=False):
        self.rng, self.rowb, self.lit_any = rng, rowb, lit_any
        self.out = bytearray()
        self.tok = []

    @property
    def pos(self):
        return len(self.out)

    def _byte(self, p):
        if p % self.rowb == 0 or not self.lit_any:
            return int(self.rng.integers(0, 5))
        return int(self.rng.integers(144, 256)) if self.rng.random() < 0.5 else int(self.rng.integers(0, 144))

    def lit(self, n=1):
        for _ in range(n):
            self.put(self._byte(self.pos))

    def put(self, b):
        assert b <= 4 or (self.lit_any and self.pos % self.rowb)
        self.tok.append(b)
        self.out.append(b)

    def raw(self, n):
        """n bytes for a stored block (not tokens)"""
        data = bytes(self._byte(self.pos + i) for i in range(n))
        self.out += data
        return data

    def _bad(self, length, dist):
        """the first row start inside the match that would receive a byte above 4"""
        first = -(-self.pos // self.rowb) * self.rowb
        for p in range(first, self.pos + length, self.rowb):
            if self.out[self.pos - dist + (p - self.pos) % dist] > 4:
                return p
        return None

    def match(self, length, dist, via284=False):
        assert dist <= self.pos
        while True:
            p = self._bad(length, dist)
            if p is None:
                break
            self.fill_to(p)
            self.lit()
        t = (length, dist, True) if via284 else (length, dist)
        self.tok.append(t)
        D.expand(self.out, [t])

    def fill_to(self, target):
        """matches of random small distances (and literals where no match fits) up to output position `target`"""
        while self.pos < target:
            n = min(258, target - self.pos)
            if target - self.pos - n in (1, 2):
                n -= 3                                          # (leave at least a match for the rest)
            if n >= 3 and self.pos >= 1:
                d = int(self.rng.integers(1, min(self.pos, 400) + 1))
                p = self._bad(n, d)
                if p is not None:
                    n = p - self.pos
                if n >= 3:
                    self.tok.append((n, d))
                    D.expand(self.out, [(n, d)])
                    continue
            self.lit()

    def take(self):
        t, self.tok = self.tok, []
        return t


class Case:
    """a valid file: .png, its geometry, .raw (the inflated bytes), .expect (the samples), .feat (what the writer recorded)"""

    def __init__(self, name, W, H, depth, ctype, stream, gen=None):
        self.name, self.W, self.H, self.depth, self.ctype = name, W, H, depth, ctype
        self.channels = 3 if ctype == 2 else 1
        self.bpp = self.channels * depth // 8
        self.rowb = 1 + W * self.bpp
        self.raw = bytes(stream.out)
        assert gen is None or bytes(gen.out) == self.raw, "generator and stream disagree"
        assert len(self.raw) == H * self.rowb, (len(self.raw), H, self.rowb)
        self.body = stream.getvalue()
        self.z = D.zlib_wrap(self.body, self.raw)
        self.png = D.png_wrap(self.z, W, H, depth, ctype)
        self.expect = D.samples(D.unfilter(self.raw, H, self.rowb, self.bpp), W, depth, self.channels)
        self.expect.setflags(write=False)
        self.feat = stream.feat
        self.blocks = list(stream.blocks)       # (kind, first output byte, bit position of the header)

    def straddles(self):
        """how many scanline ends each match runs across: the set of counts"""
        return {(pos + length - 1) // self.rowb - pos // self.rowb for pos, length, _ in self.feat["matches"]}


# ----------------------------------------------------------------------------------------------------------- valid streams
def _plan_every_symbol(g, need):
    """Tokens that use every length symbol and every distance symbol at both ends of its extra-bit range, 258 both ways,
    257, 3, the distances 1, 2, 3, 32767, 32768, and then fill the picture."""
    g.lit(40)
    small = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33)
    k = 0
    for s in range(29):
        for ex in sorted({0, (1 << D.LEN_EXTRA[s]) - 1}):
            length = D.LEN_BASE[s] + ex
            g.lit(2)
            g.match(length, small[k % len(small)], via284=(s == 27 and length == 258))
            k += 1
    g.lit(1)
    g.match(257, 2)
    g.lit(1)
    g.match(3, 1)
    g.match(258, 3)
    pending = sorted({D.DIST_BASE[s] + e for s in range(30) for e in (0, (1 << D.DIST_EXTRA[s]) - 1)} | {32767})
    lens = (3, 258, 64, 17, 130, 5)
    while pending:
        if pending[0] <= g.pos:
            g.lit(1)
            g.match(lens[len(pending) % len(lens)], pending.pop(0))
        else:
            g.lit(3)
            g.match(258, int(g.rng.integers(1, g.pos + 1)))
    assert g.pos <= need - 3, (g.pos, need)
    g.fill_to(need)


@functools.lru_cache(maxsize=None)
def long_codes():
    """16-bit gray 17 x 1217 (scanlines of 35 bytes, 42 595 bytes inflated): ONE dynamic block whose two codes are complete and
    15 deep, every symbol of both alphabets used."""
    rng = np.random.default_rng(101)
    W, H = 17, 1217
    g = Gen(rng, 1 + 2 * W)
    _plan_every_symbol(g, H * (1 + 2 * W))
    tokens = g.take()
    ls, ds = D.symbols_of(tokens)
    assert ls == set(range(5)) | set(range(256, 286)) and ds == set(range(30))
    llens = D.spread_lengths(ls, 286, 15, rng, first_split=9)
    dlens = D.spread_lengths(ds, 30, 15, rng, first_split=8)
    s = D.Deflate()
    s.dynamic(tokens, llens, dlens, final=True, cl_seq=D.rle(llens + dlens))
    return Case("long_codes", W, H, 16, 0, s, g)


@functools.lru_cache(maxsize=None)
def fixed_same():
    """The same token plan through ONE fixed block: 16-bit gray 8191 x 3 (scanlines of 16383 bytes), literals off the row
    starts from 0..255."""
    rng = np.random.default_rng(102)
    W, H = 8191, 3
    g = Gen(rng, 1 + 2 * W, lit_any=True)
    _plan_every_symbol(g, H * (1 + 2 * W))
    s = D.Deflate()
    s.fixed(g.take(), final=True)
    return Case("fixed_same", W, H, 16, 0, s, g)


OVERLAP_DISTS = (1, 2, 3, 63, 64, 65, 257)
OVERLAP_LENS = (3, 64, 65, 258)


@functools.lru_cache(maxsize=None)
def overlap():
    """8-bit gray 60 x H: every distance of OVERLAP_DISTS with every length of OVERLAP_LENS, dist == len, dist == len + 1.  The
    bytes a short-period match repeats are 1, 2, 3: never what an unwritten window would hold."""
    rng = np.random.default_rng(103)
    W = 60
    g = Gen(rng, 1 + W)
    g.lit(300)
    pairs = [(d, l) for d in OVERLAP_DISTS for l in OVERLAP_LENS] + [(l, l) for l in OVERLAP_LENS] + [(l + 1, l) for l in OVERLAP_LENS]
    for d, l in pairs:
        g.lit(2)
        for b in (1, 2, 3):
            g.put(b)
        g.match(l, d)
    H = -(-(g.pos + 3) // (1 + W))
    g.fill_to(H * (1 + W))
    tokens = g.take()
    ls, ds = D.symbols_of(tokens)
    s = D.Deflate()
    s.dynamic(tokens, D.spread_lengths(ls, 286, 9, rng), D.spread_lengths(ds, 30, 6, rng), final=True)
    return Case("overlap", W, H, 8, 0, s, g)


def _dyn(s, g, rng, final=False, depth=12):
    tokens = g.take()
    ls, ds = D.symbols_of(tokens)
    llens = D.spread_lengths(ls, 286, depth, rng)
    dlens = D.spread_lengths(ds, 30, depth, rng) if ds else [0]
    s.dynamic(tokens, llens, dlens, final=final, cl_seq=D.rle(llens + dlens))


@functools.lru_cache(maxsize=None)
def block_sequence():
    """16-bit gray 1217 x 30 (73 050 bytes): stored(0), dynamic, stored(1000), stored(0), fixed, stored(65535), dynamic (final).
    The fixed block copies out of the 1000-byte stored block and out of the dynamic block before it, the last block out of the
    65535-byte stored block, at distances up to 32768."""
    rng = np.random.default_rng(104)
    W, H = 1217, 30
    rowb = 1 + 2 * W
    g = Gen(rng, rowb)
    s = D.Deflate()
    s.stored(b"")
    g.lit(60)
    for l, d in ((3, 1), (17, 40), (258, 7), (100, 60)):
        g.lit(2)
        g.match(l, d)
    _dyn(s, g, rng)
    a_end = g.pos
    s.stored(g.raw(1000))
    s.stored(b"")
    g.match(50, 30)                         # source entirely in the stored block
    g.match(258, 1000)                      # starts at the stored block's first byte
    g.lit(3)
    g.match(40, g.pos - a_end + 20)         # starts in the dynamic block, runs into the stored one
    g.match(9, g.pos)                       # the very first byte of the stream
    s.fixed(g.take())
    s.stored(g.raw(65535))
    g.match(258, 5)                         # the stored block's last bytes
    g.lit(2)
    g.match(200, 32768)
    g.match(77, 30000)
    g.fill_to(H * rowb)
    _dyn(s, g, rng, final=True)
    return Case("block_sequence", W, H, 16, 0, s, g)


@functools.lru_cache(maxsize=None)
def stored_offsets():
    """8-bit gray 40 x H: eight stored blocks whose 3 header bits begin at bit 0, 1, .. 7 of a byte (fixed blocks of 10 and
    of 31 bits in front shift the position), a fixed block copying out of the last one."""
    rng = np.random.default_rng(105)
    W = 40
    g = Gen(rng, 1 + W)
    s = D.Deflate()
    for k in range(8):
        while s.w.bitpos % 8 != k:
            if (k - s.w.bitpos) % 2:
                g.lit(1)
                g.match(11, 1)              # 3 + 8 + (7 + 1 + 5) + 7 = 31 bits
            s.fixed(g.take())               # (empty: 3 + 7 = 10 bits)
        s.stored(g.raw(23))
    g.match(20, 21)
    H = -(-(g.pos + 3) // (1 + W))
    g.fill_to(H * (1 + W))
    s.fixed(g.take(), final=True)
    return Case("stored_offsets", W, H, 8, 0, s, g)


@functools.lru_cache(maxsize=None)
def header_seams():
    """8-bit gray 30 x H: one dynamic block per header construct (the block's letter is its index in feat['runs'])."""
    rng = np.random.default_rng(106)
    W = 30
    g = Gen(rng, 1 + W)
    s = D.Deflate()
    # a: nlen = 286, ndist = 30, an 18-run of 30 zeros from length 261 of the literal/length code to length 4 of the distance code
    g.lit(40)
    for l, d in ((3, 7), (4, 9), (5, 13), (6, 40), (4, 8)):
        g.lit(1)
        g.match(l, d)
    t = g.take()
    ls, _ = D.symbols_of(t)
    assert max(ls) == 260
    llens = D.spread_lengths(ls, 286, 6, rng)
    dlens = [0] * 5 + D.spread_lengths(range(25), 25, 8, rng)
    s.dynamic(t, llens, dlens, cl_seq=D.rle(llens[:261]) + [(18, 30)] + D.plain(dlens[5:]))
    # b: a 16-run of 5 from length 284 of the literal/length code to length 2 of the distance code
    for b in range(5):
        g.put(b)
    for l, d in ((195, 1), (227, 2), (258, 3), (250, 4)):
        g.lit(2)
        g.match(l, d)
    t = g.take()
    ls, ds = D.symbols_of(t)
    assert ls == set(range(5)) | {256, 283, 284, 285} and ds == {0, 1, 2, 3}
    llens = [0] * 286
    for sym, l in zip((0, 1, 2, 3, 4, 256, 283, 284, 285), (3, 4, 5, 6, 7, 7, 2, 2, 2)):
        llens[sym] = l
    dlens = [2, 2, 2, 2]
    s.dynamic(t, llens, dlens, cl_seq=D.rle(llens[:284]) + [(16, 5), 2])
    # c: 16 right after a 17-run and right after an 18-run (it repeats the run's 0); one distance code of length 1
    g.lit(10)
    g.match(3, 1)
    t = g.take()
    llens = D.spread_lengths(set(range(5)) | {256, 257}, 258, 5, rng)
    s.dynamic(t, llens, [1], cl_seq=D.plain(llens[:5]) + [(17, 3), (16, 3), (18, 100), (16, 6)] + D.rle(llens[117:]) + [1])
    # d: 16 repeating a non-zero length six times
    g.lit(4)
    g.match(3, 8)
    t = g.take()
    llens = D.spread_lengths(set(range(5)) | {256, 257}, 258, 5, rng)
    s.dynamic(t, llens, [3] * 8, cl_seq=D.rle(llens) + [3, (16, 6), 3])
    # e: HLIT = 257 (no length code) and no distance code (one length, 0)
    g.lit(12)
    t = g.take()
    llens = D.spread_lengths(set(range(5)) | {256}, 257, 4, rng)
    s.dynamic(t, llens, [0], cl_seq=D.rle(llens + [0]))
    # f: exactly one distance code, of length 1, for symbol 4 (distances 5 and 6: one extra bit)
    g.lit(3)
    g.match(6, 5)
    g.match(9, 6)
    t = g.take()
    llens = D.spread_lengths(D.symbols_of(t)[0], 286, 5, rng)
    s.dynamic(t, llens, [0, 0, 0, 0, 1], cl_seq=D.rle(llens + [0, 0, 0, 0, 1]))
    # g: HCLEN = 5, the fewest that can describe a block: the code-length code's lengths come in the order 16, 17, 18, 0, 8, ..
    # and a block needs a non-zero length for its end-of-block code, so with HCLEN = 4 (only 16, 17, 18, 0) no valid block exists
    # (refusals() has that one).  Here: 0 and 8 with one bit each; literals 0..254 and 256 with 8 bits, no distance code.
    g.lit(9)
    t = g.take()
    cl = [0] * 19
    cl[0] = cl[8] = 1
    llens = [8] * 255 + [0, 8]
    s.dynamic(t, llens, [0], cl_seq=D.plain(llens + [0]), cl_lens=cl)
    # h: an empty block whose only literal/length code is the end-of-block code, one bit long
    s.dynamic([], [0] * 256 + [1], [0], cl_seq=D.rle([0] * 256 + [1, 0]))
    # the rest of the picture
    H = -(-(g.pos + 3) // (1 + W))
    g.fill_to(H * (1 + W))
    _dyn(s, g, rng, final=True, depth=7)
    return Case("header_seams", W, H, 8, 0, s, g)


@functools.lru_cache(maxsize=None)
def paeth_tie_picture():
    """8-bit gray 40 x 8 of few levels ten apart, with one planted pb == pc < pa: the picture and its tie counts on the
    reference unfilter (each at least 1)"""
    rng = np.random.default_rng(11)
    H, W = 8, 40
    a = (rng.integers(0, 6, (H, W)) * 10 + 60).astype(np.uint8)
    a[2, 10:12] = (100, 80)                 # c = 100 and b = 80 above, a = 110 to the left:
    a[3, 10] = 110                          # p = 90, pa = 20, pb = pc = 10 -> the predictor is b, not c
    ties = {}
    assert np.array_equal(D.unfilter(D._filter_rows(a, 1, (4,)), H, 1 + W, 1, ties), a)
    assert min(ties.get(k, 0) for k in ("pa==pb", "pb==pc", "all")) >= 1, ties
    a.setflags(write=False)
    return a, ties


VALID = (long_codes, fixed_same, overlap, block_sequence, stored_offsets, header_seams)


# ----------------------------------------------------------------------------------------------------------------- refusals
class Refusal:
    """a file the decoder must refuse: .png, the call's geometry and output kind, the status, the substring of zlib's message
    (None where the stream itself is valid and the PNG layer refuses), and the check in png_kernels.hip that ends it"""

    def __init__(self, row, name, png, status, zmsg, why, W=7, H=3, channels=1, want="disp", z=None, raw=b"", rows=0):
        self.row, self.name, self.png, self.status, self.zmsg, self.why = row, name, png, status, zmsg, why
        self.W, self.H, self.channels, self.want, self.z = W, H, channels, want, z
        self.raw, self.rows = raw, rows     # the inflated bytes; the scanlines written before the refusal

    @property
    def id(self):
        return "row%s-%s" % (self.row, self.name)


RW, RH = 7, 3           # the refusals' picture: 8-bit gray 7 x 3, scanlines of 8 bytes, 24 bytes inflated
RNEED = (1 + RW) * RH
LL_OK = [2, 2, 2, 3, 4] + [0] * 251 + [4, 0]        # literals 0..4 and end-of-block, complete; 257 exists (length 0) for edits
DL_OK = [1, 1]


def _raw_ok(n=RNEED, rng=None):
    rng = rng or np.random.default_rng(7)
    return bytes(int(v) for v in rng.integers(0, 5, n))


def _wrap(body, raw=b"", W=RW, H=RH, depth=8, ctype=0, head=b"\x78\x01"):
    z = head + body + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)
    return D.png_wrap(z, W, H, depth, ctype), z


def _header_only(llens, dlens, **kw):
    w = D.BitWriter()
    D.write_dynamic_header(w, 1, llens, dlens, **kw)
    return w.getvalue() + bytes(8)


def _fixed_syms(items):
    """a final fixed block from raw items: ('L', literal/length symbol), ('D', 5-bit distance code), ('X', value, bits)"""
    w = D.BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    lc = D.canonical(D.FIXED_LLENS)
    for it in items:
        if it[0] == "L":
            w.code(lc[it[1]], D.FIXED_LLENS[it[1]])
        elif it[0] == "D":
            w.code(it[1], 5)
        else:
            w.bits(it[1], it[2])
    return w.getvalue() + bytes(8)


@functools.lru_cache(maxsize=None)
def refusals():
    out = []

    def add(row, name, body, status, zmsg, why, raw=b"", **kw):
        png, z = _wrap(body, raw, **{k: v for k, v in kw.items() if k in ("W", "H", "depth", "ctype", "head")})
        out.append(Refusal(row, name, png, status, zmsg, why, z=z, raw=raw, **{k: v for k, v in kw.items() if k in ("channels", "want", "rows")}))

    E_HUFF_LENS = "`if (ed != 0 || el != 0)` after png_huff_build"
    ll = list(LL_OK)
    ll[5] = 1
    add(1, "litlen-oversubscribed", _header_only(ll, DL_OK), 6, "invalid literal/lengths set", E_HUFF_LENS + " returned -1 (left < 0)")
    ll = [0] * 258
    ll[0] = ll[256] = 2
    add(2, "litlen-incomplete-two-codes", _header_only(ll, DL_OK), 6, "invalid literal/lengths set", E_HUFF_LENS + " returned left > 0 with two codes")
    cl = [0] * 19
    cl[0] = cl[8] = 2
    add(3, "codelen-code-incomplete", _header_only(LL_OK, DL_OK, cl_seq=[], cl_lens=cl), 6, "invalid code lengths set",
        "`if (e != 0)` after png_huff_build of the 19 code-length lengths")
    add(4, "16-first", _header_only(LL_OK, DL_OK, cl_seq=[(16, 3)] + D.plain(LL_OK[3:] + DL_OK)), 6, "invalid bit length repeat",
        "`if (idx == 0)` in the sym == 16 branch")
    add(5, "run-past-the-end", _header_only(LL_OK, DL_OK, cl_seq=D.plain(LL_OK[:250]) + [(18, 11)]), 6, "invalid bit length repeat",
        "`if (idx + rep > nlen + ndist)`: 250 + 11 > 258 + 2")
    ll = [1, 1] + [0] * 256
    add(6, "no-end-of-block", _header_only(ll, DL_OK), 6, "missing end-of-block", "`if (sld8(cl + 256) == 0)`")
    cl = [0] * 19
    cl[16] = cl[17] = cl[18] = cl[0] = 2
    add(6, "hclen4-no-end-of-block", _header_only([0] * 257, [0], cl_seq=[(18, 138), (18, 120)], cl_lens=cl, hclen=4), 6,
        "missing end-of-block", "`if (sld8(cl + 256) == 0)`: HCLEN = 4 can only spell zeros")
    for field, n in ((30, 287), (31, 288)):
        add(7, "hlit-%d" % n, _header_only(LL_OK, DL_OK, hlit=field), 6, "too many length or distance symbols", "`if (nlen > 286 || ndist > 30)`")
    for field, n in ((30, 31), (31, 32)):
        add(7, "hdist-%d" % n, _header_only(LL_OK, DL_OK, hdist=field), 6, "too many length or distance symbols", "`if (nlen > 286 || ndist > 30)`")
    for sym in (286, 287):
        add(8, "fixed-symbol-%d" % sym, _fixed_syms([("L", 0), ("L", sym)]), 6, "invalid literal/length code", "`if (sym >= 29)` after sym -= 257")
    for code in (30, 31):
        add(8, "fixed-distance-%d" % code, _fixed_syms([("L", 0), ("L", 257), ("D", code)]), 6, "invalid distance code",
            "`if (ds < 0 || ds >= 30)`: the 30-symbol table has no entry, the walk finds no code and returns -1")
    # a length symbol where the block has no distance code
    ll = list(LL_OK)
    ll[4], ll[257] = 5, 5
    assert D.kraft(ll) == 1 << 15
    w = D.BitWriter()
    D.write_dynamic_header(w, 1, ll, [0])
    lc = D.canonical(ll)
    w.code(lc[0], ll[0])
    w.code(lc[257], ll[257])
    add(9, "length-without-distance-code", w.getvalue() + bytes(8), 6, "invalid distance code",
        "`if (ds < 0 || ds >= 30)`: an all-0xFFFF table and all-zero counts, the walk returns -1")
    w = D.BitWriter()
    D.write_dynamic_header(w, 1, ll, [2])
    w.code(lc[0], ll[0])
    w.code(lc[257], ll[257])
    w.code(0, 2)
    w.code(lc[256], ll[256])
    add(10, "one-distance-code-of-length-2", w.getvalue() + bytes(8), 6, "invalid distances set",
        "`if (ed != 0 || el != 0)`: a single code is let through only with length 1")
    add(10, "only-end-of-block-of-length-2", _header_only([0] * 256 + [2], [0]), 6, "invalid literal/lengths set",
        "`if (ed != 0 || el != 0)`: a single code is let through only with length 1")
    w = D.BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    add(11, "block-type-3", w.getvalue() + bytes(8), 5, "invalid block type", "the `else` of the block-type switch")
    s = D.Deflate()
    s.stored(_raw_ok(), final=True, nlen=0x1234)
    add(12, "stored-nlen-mismatch", s.getvalue(), 5, "invalid stored block lengths", "`if ((len ^ 0xFFFFu) != nlen)`")
    add(13, "distance-1-at-the-start", _fixed_syms([("L", 257), ("D", 0)]), 5, "invalid distance too far back", "`if (dist > wpos)`: 1 > 0")
    add(13, "distance-wpos-plus-1", _fixed_syms([("L", 0)] * 5 + [("L", 257), ("D", 4), ("X", 1, 1)]), 5, "invalid distance too far back",
        "`if (dist > wpos)`: 6 > 5")
    raw = _raw_ok()
    s = D.Deflate()
    s.fixed(list(raw), final=True)
    good = s.getvalue()
    for name, head, msg in (("cm-9", bytes([0x79, 31 - (0x7900 % 31)]), "unknown compression method"),
                            ("fdict", bytes([0x78, 0x20 + 31 - (0x7820 % 31)]), None),
                            ("fcheck", b"\x78\x02", "incorrect header check")):
        assert name == "fcheck" or (head[0] * 256 + head[1]) % 31 == 0
        add(14, name, good, 5, msg or "", "`(cmf & 15) != 8 || (flg & 32) || ((cmf << 8) | flg) % 31`", raw=raw, head=head)
    # ---- PNG-level refusals: the zlib stream is valid
    d16 = np.random.default_rng(8).integers(0, 65536, (RH, RW)).astype(np.uint16)
    rows = d16.astype(">u2").view(np.uint8).reshape(RH, RW * 2)
    raw16 = D._filter_rows(rows, 2, (0, 1, 2))
    s = D.Deflate()
    s.fixed(list(raw16), final=True)
    add(15, "gray16-into-u8", s.getvalue(), 3, None, "`if (j.out_u8 && depth != 8)` behind the IHDR checks", raw=raw16, depth=16, want="u8")
    for n, tag in ((RNEED + 1, "need+1"), (RNEED - 1, "need-1")):
        raw = _raw_ok(n)
        end = "`if ((long long)wpos != need || rows_done != (int)h)` after the last block"
        s = D.Deflate()
        s.fixed(list(raw), final=True)
        add(16, tag + "-by-literal", s.getvalue(), 4, None, "`if ((long long)wpos >= need)` at the literal" if n > RNEED else end, raw=raw,
            rows=3 if n > RNEED else 2)
        s = D.Deflate()
        s.fixed(list(raw[:n - 3]) + [(3, 1)], final=True)
        add(16, tag + "-by-match", s.getvalue(), 4, None, "`if ((long long)wpos + len > need)` at the match" if n > RNEED else end,
            raw=bytes(s.out), rows=2)
        s = D.Deflate()
        s.fixed(list(raw[:10]))
        s.stored(raw[10:], final=True)
        add(16, tag + "-by-stored", s.getvalue(), 4, None, "`if ((long long)wpos + len > need)` at LEN" if n > RNEED else end, raw=raw,
            rows=1 if n > RNEED else 2)
    for y in (0, RH - 1):
        raw = bytearray(_raw_ok())
        raw[y * (1 + RW)] = 5
        s = D.Deflate()
        s.fixed(list(raw), final=True)
        add(17, "filter-5-on-row-%d" % y, s.getvalue(), 7, None, "the last `else` of png_row's filter switch", raw=bytes(raw), rows=y)
    raw = _raw_ok()
    s = D.Deflate()
    s.fixed(list(raw), final=True)
    for ctype, depth in ((3, 8), (4, 8), (6, 8), (0, 1), (0, 2), (0, 4), (2, 16)):
        add(18, "ctype%d-depth%d" % (ctype, depth), s.getvalue(), 3, None, "the colour type / depth test behind IHDR", raw=raw, ctype=ctype,
            depth=depth, channels=3 if ctype == 2 else 1, want="u8" if ctype == 2 else "disp")
    return tuple(out)


def refusal(name):
    return next(r for r in refusals() if r.name == name)


@functools.lru_cache(maxsize=None)
def small_good_case(seed):
    """a valid 8-bit gray 7 x 3 file for the batch test"""
    rng = np.random.default_rng(seed)
    g = Gen(rng, 1 + RW)
    g.lit(9)
    g.match(5, 3)
    g.fill_to(RNEED)
    s = D.Deflate()
    s.fixed(g.take(), final=True)
    return Case("small_good_%d" % seed, RW, RH, 8, 0, s, g)


def small_good(seed):
    """(png, samples) of small_good_case"""
    c = small_good_case(seed)
    return c.png, c.expect
