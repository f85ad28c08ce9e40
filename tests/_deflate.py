"""A DEFLATE / zlib / PNG writer for tests (RFC 1951, RFC 1950, PNG 1.2): plain Python + numpy, no GPU, no library code.

zlib's and PIL's encoders decide for themselves which code lengths, match lengths and distances a stream holds; this writer
lets a test decide: it emits stored, fixed and dynamic blocks from explicit token lists, explicit code lengths and an explicit
code-length sequence, valid or not.  Every stream records which constructs it actually emitted (`Deflate.feat`), so that a
test can assert "this input reaches 15-bit distance codes" on the writer's side instead of hoping (tests/test_deflate_cpu.py).

A token is a literal byte (int) or a match `(length, distance)`; `(258, distance, True)` encodes length 258 as code 284 with
extra bits 31 instead of code 285 (both are legal, RFC 1951 3.2.5).
"""
import struct
import zlib

import numpy as np

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LLENS = tuple([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)     # 288 symbols: 286 and 287 have codes and no meaning
FIXED_DLENS = tuple([5] * 32)                                       # 32 codes: 30 and 31 have codes and no meaning


# ------------------------------------------------------------------------------------------------------------ bits and codes
class BitWriter:
    """DEFLATE's bit order: fields LSB first, Huffman codes MSB first, bytes filled from bit 0 up."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, k):
        assert 0 <= v < (1 << k), (v, k)
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, l):
        assert 0 <= c < (1 << l), (c, l)
        self.bits(int(format(c, "0%db" % l)[::-1], 2) if l else 0, l)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """RFC 1951 3.2.2: the code of every symbol with a non-zero length (None otherwise).  Lengths that over-subscribe the
    code space still get codes (masked to their length): such a header is refused before any of them is read."""
    maxl = max(list(lens) + [0])
    count = [0] * (maxl + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * (maxl + 2)
    for b in range(1, maxl + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append(nxt[l] & ((1 << l) - 1))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lens):
    """sum of 2^(15 - l) over the non-zero lengths: 2^15 = complete, more = over-subscribed, less = incomplete"""
    return sum(1 << (15 - l) for l in lens if l)


def complete_lengths(n, depth, first_split=None):
    """n code lengths of a COMPLETE code whose longest code has `depth` bits.  The chain 1, 2, .., depth - 1, depth, depth is
    complete with depth + 1 symbols; every split (one code of length l -> two of l + 1) adds a symbol and keeps it complete.
    With first_split the first split takes the only code of that length and later ones the longest length that still has two
    codes: every other length from 1 to depth stays populated.  Without it the shortest codes are split first.  Ascending."""
    if n == 1:
        return [1]
    assert depth + 1 <= n <= (1 << depth), (n, depth)
    c = [0] + [1] * depth + [0]
    c[depth] = 2
    have = depth + 1
    if have < n and first_split is not None:
        c[first_split] -= 1
        c[first_split + 1] += 2
        have += 1
    while have < n:
        cand = [l for l in range(1, depth) if c[l] >= 2]
        if cand:
            l = max(cand)
        else:
            l = min(l for l in range(1, depth) if c[l] >= 1)
        c[l] -= 1
        c[l + 1] += 2
        have += 1
    out = [l for l in range(1, depth + 1) for _ in range(c[l])]
    assert len(out) == n and kraft(out) == 1 << 15
    return out


def length_symbol(length, via284=False):
    """(symbol, extra bits, extra value) of a match length"""
    assert 3 <= length <= 258
    if length == 258 and not via284:
        return 285, 0, 0
    assert not via284 or length == 258
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    assert length - LEN_BASE[k] < (1 << LEN_EXTRA[k])
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, DIST_EXTRA[k], dist - DIST_BASE[k]


def expand(out, tokens):
    """append the plain LZ77 expansion of `tokens` to the bytearray `out`"""
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t[0], t[1]
            assert 3 <= length <= 258 and 1 <= dist <= len(out), (t, len(out))
            for _ in range(length):
                out.append(out[-dist])
        else:
            assert 0 <= t <= 255
            out.append(t)


def reference(tokens, history=b""):
    """The plain LZ77 expansion of a token list behind `history`: the bytes the tokens stand for."""
    out = bytearray(history)
    expand(out, tokens)
    return bytes(out[len(history):])


def symbols_of(tokens):
    """(literal/length symbols incl. 256, distance symbols) a token list needs"""
    ls, ds = {256}, set()
    for t in tokens:
        if isinstance(t, tuple):
            ls.add(length_symbol(t[0], len(t) > 2 and t[2])[0])
            ds.add(dist_symbol(t[1])[0])
        else:
            ls.add(t)
    return ls, ds


def spread_lengths(symbols, n_alphabet, depth, rng, first_split=None):
    """a complete code of the given depth over `symbols` (lengths dealt out in a seeded random order), 0 elsewhere"""
    symbols = sorted(symbols)
    lens = complete_lengths(len(symbols), min(depth, max(1, len(symbols) - 1)), first_split)
    perm = rng.permutation(len(symbols))
    out = [0] * n_alphabet
    for k, l in zip(perm, lens):
        out[symbols[k]] = l
    return out


# ------------------------------------------------------------------------------------------------- code-length sequences
def plain(lens):
    """the code-length sequence that spells every length out (no runs)"""
    return list(lens)


def rle(lens):
    """a greedy run-length coding of a list of code lengths: 17 / 18 for zeros, 16 for repeats"""
    out, i, n = [], 0, len(lens)
    while i < n:
        j = i
        while j < n and lens[j] == lens[i]:
            j += 1
        run = j - i
        if lens[i] == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k))
                run -= k
            if run >= 3:
                out.append((17, run))
                run = 0
            out += [0] * run
        else:
            out.append(lens[i])
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k))
                run -= k
            out += [lens[i]] * run
        i = j
    return out


def expand_cl_seq(seq):
    """what a decoder makes of a code-length sequence, and where its runs fell: [(symbol, first index, count, symbol before)]"""
    out, runs, before = [], [], None
    for it in seq:
        if isinstance(it, tuple):
            sym, n = it
            lo, hi = {16: (3, 6), 17: (3, 10), 18: (11, 138)}[sym]
            assert lo <= n <= hi, it
            runs.append((sym, len(out), n, before))
            out += [out[-1] if sym == 16 else 0] * n
            before = sym
        else:
            assert 0 <= it <= 15
            out.append(it)
            before = it
    return out, runs


DEFAULT_CL_LENS = tuple([4] * 13 + [5] * 6)     # a complete code over all 19 symbols: HCLEN = 19


def write_dynamic_header(w, final, llens, dlens, cl_seq=None, cl_lens=None, hclen=None, hlit=None, hdist=None):
    """The header of a dynamic block (RFC 1951 3.2.7), valid or not: nothing is checked here.  Returns the runs of the
    code-length sequence (expand_cl_seq)."""
    seq = plain(list(llens) + list(dlens)) if cl_seq is None else cl_seq
    cl_lens = list(DEFAULT_CL_LENS if cl_lens is None else cl_lens)
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
    w.bits(final, 1)
    w.bits(2, 2)
    w.bits(len(llens) - 257 if hlit is None else hlit, 5)
    w.bits(len(dlens) - 1 if hdist is None else hdist, 5)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl_lens[CL_ORDER[i]], 3)
    codes = canonical(cl_lens)
    runs, idx, before = [], 0, None
    for it in seq:
        sym, n = it if isinstance(it, tuple) else (it, None)
        assert cl_lens[sym], "code-length symbol %d has no code" % sym
        w.code(codes[sym], cl_lens[sym])
        if sym >= 16:
            lo, nb = {16: (3, 2), 17: (3, 3), 18: (11, 7)}[sym]
            w.bits(n - lo, nb)
            runs.append((sym, idx, n, before))
            idx += n
        else:
            idx += 1
        before = sym
    return runs


# --------------------------------------------------------------------------------------------------------------- the stream
class Deflate:
    """A raw DEFLATE stream under construction.  `out` is what it inflates to so far (the reference expansion of every
    block's tokens), `feat` what it used."""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()
        self.blocks = []            # (kind, first output byte, bit position of the header)
        self.feat = {
            "lit_code_lens": {"fixed": set(), "dynamic": set()},    # code lengths of the literal/length symbols emitted
            "dist_code_lens": {"fixed": set(), "dynamic": set()},
            "len_syms": set(), "dist_syms": set(),
            "dist_extra": {},                                       # distance symbol -> extra values emitted
            "len_extra": {},
            "lengths": set(), "distances": set(),
            "pairs": set(),                                         # (distance, length)
            "periods": set(),                                       # distance of matches with distance < length
            "literals": set(),
            "matches": [],                                          # (output position, length, distance)
            "cross": set(),                                         # (kind of the block, kind of the block its source starts in)
            "stored_bit_offsets": set(), "stored_lens": set(),
            "runs": [],                                             # per dynamic header: (nlen, ndist, runs of expand_cl_seq)
            "codes": [],                                            # per dynamic header: (llens, dlens)
            "hclen": set(), "nlen": set(), "ndist": set(),
        }

    def _kind_at(self, pos):
        kind = None
        for k, start, _ in self.blocks:
            if start <= pos:
                kind = k
        return kind

    def stored(self, data, final=False, nlen=None):
        self.blocks.append(("stored", len(self.out), self.w.bitpos))
        self.feat["stored_bit_offsets"].add(self.w.bitpos % 8)
        self.feat["stored_lens"].add(len(data))
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.w.raw(bytes(data))
        self.out += data

    def _tokens(self, kind, tokens, llens, dlens, eob=True):
        lc, dc = canonical(llens), canonical(dlens)
        f, w = self.feat, self.w
        start = len(self.out)
        for t in tokens:
            if isinstance(t, tuple):
                length, dist = t[0], t[1]
                ls, lb, lv = length_symbol(length, len(t) > 2 and t[2])
                ds, db, dv = dist_symbol(dist)
                assert llens[ls] and dlens[ds], ("no code for", t)
                w.code(lc[ls], llens[ls])
                w.bits(lv, lb)
                w.code(dc[ds], dlens[ds])
                w.bits(dv, db)
                pos = len(self.out)
                f["lit_code_lens"][kind].add(llens[ls])
                f["dist_code_lens"][kind].add(dlens[ds])
                f["len_syms"].add(ls)
                f["dist_syms"].add(ds)
                f["dist_extra"].setdefault(ds, set()).add(dv)
                f["len_extra"].setdefault(ls, set()).add(lv)
                f["lengths"].add(length)
                f["distances"].add(dist)
                f["pairs"].add((dist, length))
                if dist < length:
                    f["periods"].add(dist)
                f["matches"].append((pos, length, dist))
                if pos - dist < start:
                    f["cross"].add((kind, self._kind_at(pos - dist)))
                expand(self.out, [t])
            else:
                assert llens[t], ("no code for literal", t)
                w.code(lc[t], llens[t])
                f["lit_code_lens"][kind].add(llens[t])
                f["literals"].add(t)
                self.out.append(t)
        if eob:
            w.code(lc[256], llens[256])
            f["lit_code_lens"][kind].add(llens[256])

    def fixed(self, tokens, final=False):
        self.blocks.append(("fixed", len(self.out), self.w.bitpos))
        self.w.bits(int(final), 1)
        self.w.bits(1, 2)
        self._tokens("fixed", tokens, FIXED_LLENS, FIXED_DLENS)

    def dynamic(self, tokens, llens, dlens, final=False, cl_seq=None, cl_lens=None, hclen=None):
        """a VALID dynamic block: the lengths must form what RFC 1951 and zlib accept, and an explicit code-length sequence
        must spell exactly llens + dlens"""
        assert 257 <= len(llens) <= 286 and 1 <= len(dlens) <= 30 and llens[256]
        nl, nd = sum(1 for l in llens if l), sum(1 for l in dlens if l)
        assert kraft(llens) == 1 << 15 or (nl == 1 and max(llens) == 1), "literal/length code not complete"
        assert nd == 0 or kraft(dlens) == 1 << 15 or (nd == 1 and max(dlens) == 1), "distance code not complete"
        if cl_seq is not None:
            assert expand_cl_seq(cl_seq)[0] == list(llens) + list(dlens), "the sequence does not spell the lengths"
        if cl_lens is not None:
            assert kraft(cl_lens) == 1 << 15 and max(cl_lens) <= 7
        self.blocks.append(("dynamic", len(self.out), self.w.bitpos))
        before = self.w.bitpos
        runs = write_dynamic_header(self.w, int(final), llens, dlens, cl_seq, cl_lens, hclen)
        self.feat["runs"].append((len(llens), len(dlens), runs))
        self.feat["codes"].append((tuple(llens), tuple(dlens)))
        self.feat["nlen"].add(len(llens))
        self.feat["ndist"].add(len(dlens))
        hc = hclen if hclen is not None else max([4] + [i + 1 for i in range(19) if (cl_lens or DEFAULT_CL_LENS)[CL_ORDER[i]]])
        self.feat["hclen"].add(hc)
        assert self.w.bitpos > before
        self._tokens("dynamic", tokens, llens, dlens)

    def getvalue(self):
        return self.w.getvalue()


def zlib_wrap(body, raw):
    """RFC 1950: header 78 01 (CM = 8, 32 KB window, no dictionary, check bits) + the raw DEFLATE stream + Adler-32 of `raw`"""
    return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)


# --------------------------------------------------------------------------------------------------------------------- PNG
PNG_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _ihdr(W, H, depth, ctype, interlace=0):
    return _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, interlace))


def png_wrap(zstream, W, H, depth, ctype, idat_split=(1 << 30,)):
    """a PNG file around a finished zlib stream"""
    out = PNG_SIG + _ihdr(W, H, depth, ctype)
    pos, k = 0, 0
    while pos < len(zstream):
        n = idat_split[k % len(idat_split)]
        out += _chunk(b"IDAT", zstream[pos:pos + n])
        pos += n
        k += 1
    return out + _chunk(b"IEND", b"")


def _filter_rows(img_bytes, bpp, types):
    """img_bytes: [H, rowbytes] uint8 -> filtered scanlines (PNG spec 9.2) with the given filter type per row."""
    H, nb = img_bytes.shape
    out = bytearray()
    prev = np.zeros(nb, np.int32)
    for y in range(H):
        cur = img_bytes[y].astype(np.int32)
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
        t = types[y % len(types)]
        if t == 0:
            f = cur
        elif t == 1:
            f = cur - a
        elif t == 2:
            f = cur - prev
        elif t == 3:
            f = cur - ((a + prev) >> 1)
        else:
            p = a + prev - c
            pa, pb, pc = np.abs(p - a), np.abs(p - prev), np.abs(p - c)
            pr = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
            f = cur - pr
        out.append(t)
        out += (f & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def _raw_png(arr, types=(0, 1, 2, 3, 4), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, idat_split=(1 << 30,), extra=True):
    """hand-rolled PNG writer: explicit filter types, zlib strategy and IDAT chunking"""
    H, W = arr.shape[:2]
    if arr.dtype == np.uint16:
        depth, ctype, bpp = 16, 0, 2
        rows = arr.astype(">u2").view(np.uint8).reshape(H, W * 2)
    elif arr.ndim == 3:
        depth, ctype, bpp = 8, 2, 3
        rows = arr.reshape(H, W * 3)
    else:
        depth, ctype, bpp = 8, 0, 1
        rows = arr.reshape(H, W)
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    z = co.compress(_filter_rows(rows, bpp, types)) + co.flush()
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, 0))
    if extra:
        out += _chunk(b"tEXt", b"Comment\x00ancillary chunk before the image data") + _chunk(b"pHYs", struct.pack(">IIB", 1, 1, 0))
    pos, k = 0, 0
    while pos < len(z):
        n = idat_split[k % len(idat_split)]
        out += _chunk(b"IDAT", z[pos:pos + n])
        if k == 1:
            out += _chunk(b"IDAT", b"")  # an empty IDAT chunk is legal
        pos += n
        k += 1
    return out + _chunk(b"IEND", b"")


def paeth_predictor(a, b, c):
    """PNG spec 9.4, as written there"""
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    if pb <= pc:
        return b
    return c


def unfilter(raw, H, rowb, bpp, ties=None):
    """The inverse of _filter_rows, scalar and obvious (PNG spec 9.2): inflated bytes -> [H, rowb - 1] uint8.  `ties`, if a
    dict, counts the Paeth ties: pa == pb alone, pb == pc < pa between different bytes (the one a `<` for the `<=` gets
    wrong), all three equal."""
    assert len(raw) == H * rowb
    nb = rowb - 1
    out = np.zeros((H, nb), np.uint8)
    prev = [0] * nb
    for y in range(H):
        ft = raw[y * rowb]
        f = raw[y * rowb + 1:(y + 1) * rowb]
        cur = [0] * nb
        if ft == 0:
            cur = list(f)
        elif ft == 1:
            for i in range(nb):
                cur[i] = (f[i] + (cur[i - bpp] if i >= bpp else 0)) & 255
        elif ft == 2:
            for i in range(nb):
                cur[i] = (f[i] + prev[i]) & 255
        elif ft == 3:
            for i in range(nb):
                cur[i] = (f[i] + (((cur[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)) & 255
        elif ft == 4:
            for i in range(nb):
                a, b, c = (cur[i - bpp], prev[i], prev[i - bpp]) if i >= bpp else (0, prev[i], 0)
                if ties is not None:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    if pa == pb and pa != pc:   # (|b - c| == |a - c| means a == b or pc == 0: the tie never decides between values)
                        ties["pa==pb"] = ties.get("pa==pb", 0) + 1
                    if pb == pc and pb < pa and b != c:
                        ties["pb==pc"] = ties.get("pb==pc", 0) + 1
                    if pa == pb == pc:
                        ties["all"] = ties.get("all", 0) + 1
                cur[i] = (f[i] + paeth_predictor(a, b, c)) & 255
        else:
            raise ValueError("filter type %d on row %d" % (ft, y))
        out[y] = cur
        prev = cur
    return out


def samples(rows, W, depth, channels):
    """unfiltered scanline bytes -> the samples: [H, W] uint16 / uint8 for gray, [H, W, 3] uint8 for RGB"""
    H = rows.shape[0]
    if depth == 16:
        assert channels == 1
        return np.ascontiguousarray(rows).view(">u2").astype(np.uint16).reshape(H, W)
    return rows.reshape(H, W) if channels == 1 else rows.reshape(H, W, 3)
