"""Deflate / BGZF tools for the inflate tests (CPU only).  The yardstick is Python's zlib.

(a) bgzf_member wraps a raw deflate stream as a BGZF block;
(b) walk is a pure-Python walker of a deflate stream: the text and what the stream is made of;
(c) fixed_stream writes a fixed-Huffman stream from a token list -- zlib never emits a distance above 32,506, so the
    edge cases are assembled by hand;
and the three fixture sets built from them: valid_fixtures(), damaged_fixtures(), flip_fixtures().
"""
import functools
import random
import struct
import zlib

OK, HEADER, DATA, SIZE, CRC = 0, 1, 2, 3, 4
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def bgzf_member(deflate_bytes, text, extra=b"", extra_after=b""):
    """a BGZF block around a raw deflate stream (as tests/test_cli_virtual_gpus.py::_write_bgzf lays it out); `extra` /
    `extra_after`: whole extra subfields before / after BC"""
    xlen = 6 + len(extra) + len(extra_after)
    total = 12 + xlen + len(deflate_bytes) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\0" + struct.pack("<H", total - 1)
            + extra_after + deflate_bytes + struct.pack("<II", zlib.crc32(text), len(text) & 0xFFFFFFFF))


def deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(text) + co.flush()


# ---- (b) the walker ------------------------------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


class _Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0  # pos in bits

    def take(self, n):
        v = 0
        for k in range(n):
            byte = self.data[self.pos >> 3]  # IndexError past the end
            v |= ((byte >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _canonical(lengths):
    """{(length, code): symbol}"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[(l, nxt[l])] = s
            nxt[l] += 1
    return out


def _symbol(bits, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (l, code) in table:
            return table[(l, code)]
    raise ValueError("no code matches")


def walk(stream):
    """(text, tallies) of a raw deflate stream: types (set), blocks, empty_stored, max_code_len, max_match, max_dist,
    overlapping (matches with dist < len), match_258_at_1"""
    bits, out = _Bits(stream), bytearray()
    t = dict(types=set(), blocks=0, empty_stored=0, max_code_len=0, max_match=0, max_dist=0, overlapping=0, match_258_at_1=0)
    last = 0
    while not last:
        last, kind = bits.take(1), bits.take(2)
        t["types"].add(kind)
        t["blocks"] += 1
        if kind == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            if n ^ 0xFFFF != nn:
                raise ValueError("stored lengths disagree")
            at = bits.pos >> 3
            if at + n > len(stream):
                raise ValueError("stored block past the end")
            out += stream[at:at + n]
            bits.pos += 8 * n
            t["empty_stored"] += n == 0
            continue
        if kind == 3:
            raise ValueError("block type 3")
        if kind == 1:
            lit, dist = _canonical(FIXED_LIT), _canonical([5] * 32)
            t["max_code_len"] = max(t["max_code_len"], 9)
        else:
            hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
            cl = [0] * 19
            for k in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][:hclen]:
                cl[k] = bits.take(3)
            clt, lens = _canonical(cl), []
            while len(lens) < hlit + hdist:
                s = _symbol(bits, clt)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + bits.take(2))
                elif s == 17:
                    lens += [0] * (3 + bits.take(3))
                else:
                    lens += [0] * (11 + bits.take(7))
            if len(lens) != hlit + hdist:
                raise ValueError("code lengths overrun")
            lit, dist = _canonical(lens[:hlit]), _canonical(lens[hlit:])
            t["max_code_len"] = max([t["max_code_len"]] + lens)
        while True:
            s = _symbol(bits, lit)
            if s < 256:
                out.append(s)
            elif s == 256:
                break
            else:
                if s > 285:
                    raise ValueError("literal/length symbol beyond 285")
                n = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                ds = _symbol(bits, dist)
                if ds > 29:
                    raise ValueError("distance symbol beyond 29")
                d = DIST_BASE[ds] + bits.take(DIST_EXTRA[ds])
                if d > len(out):
                    raise ValueError("distance beyond the text")
                for _ in range(n):
                    out.append(out[-d])
                t["max_match"], t["max_dist"] = max(t["max_match"], n), max(t["max_dist"], d)
                t["overlapping"] += d < n
                t["match_258_at_1"] += (n, d) == (258, 1)
    return bytes(out), t


# ---- (c) the fixed-Huffman writer ------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):  # n bits of v, least significant first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):  # a Huffman code: most significant bit first
        self.put(int(format(c, "0%db" % n)[::-1], 2), n)

    def done(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def _fixed_lit(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


def fixed_stream(tokens, final=True, raw_lit=None, raw_dist=None):
    """one fixed-Huffman block from literals (ints) and (len, dist) tokens.  raw_lit / raw_dist: a literal/length symbol
    and a distance symbol appended before the end-of-block code as they are (for the damaged set)"""
    w = BitWriter()
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            _fixed_lit(w, t)
            continue
        n, d = t
        ls = max(k for k in range(29) if LEN_BASE[k] <= n and (k == 28 or n < 258))
        _fixed_lit(w, 257 + ls)
        w.put(n - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = max(k for k in range(30) if DIST_BASE[k] <= d)
        w.code(ds, 5)
        w.put(d - DIST_BASE[ds], DIST_EXTRA[ds])
    if raw_lit is not None:
        _fixed_lit(w, raw_lit)
    if raw_dist is not None:
        _fixed_lit(w, 257)
        w.code(raw_dist, 5)
    _fixed_lit(w, 256)
    return w.done()


def tokens_text(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


# ---- fixtures --------------------------------------------------------------------------------------------------------
def fastq_text(n_bytes, seed=7):
    rng, out, k = random.Random(seed), bytearray(), 0
    while len(out) < n_bytes:
        seq = "".join(rng.choice("ACGT") for _ in range(100))
        qual = "".join(rng.choice("FFFFFFF:,#") for _ in range(100))
        out += ("@SRR0000001.%d %d/1\n%s\n+\n%s\n" % (k, k, seq, qual)).encode()
        k += 1
    return bytes(out[:n_bytes])


@functools.lru_cache(maxsize=None)
def valid_fixtures():
    """[(name, member bytes, text)] -- every one a block zlib inflates"""
    fq = fastq_text(65280)
    out = []

    def add(name, stream, text, **kw):
        out.append((name, bgzf_member(stream, text, **kw), text))

    for level in (1, 6, 9):
        add("fastq level %d" % level, deflate(fq, level), fq)
    add("fastq Z_FIXED", deflate(fq, 6, zlib.Z_FIXED), fq)
    add("fastq level 0", deflate(fq, 0), fq)
    add("fastq Z_HUFFMAN_ONLY", deflate(fq, 6, zlib.Z_HUFFMAN_ONLY), fq)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    third = len(fq) // 3
    z = co.compress(fq[:third]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(fq[third:2 * third]) + co.flush(zlib.Z_SYNC_FLUSH)
    add("fastq flushed twice", z + co.compress(fq[2 * third:]) + co.flush(), fq)
    zeros = bytes(65280)
    add("zeros", deflate(zeros), zeros)
    rng = random.Random(3)
    fib, letters = [1, 1], []
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    for k, f in enumerate(fib):
        letters += [65 + k] * f
    rng.shuffle(letters)
    fibs = bytes(letters)[:65280]
    add("fibonacci frequencies", deflate(fibs, 6, zlib.Z_HUFFMAN_ONLY), fibs)
    fq2 = fastq_text(65535, seed=11)
    add("fastq 65535 level 1", deflate(fq2, 1), fq2)
    add("one byte", deflate(b"x"), b"x")
    rnd = bytes(rng.getrandbits(8) for _ in range(30000))
    add("random bytes", deflate(rnd), rnd)
    # hand-assembled: a literal prefix long enough for the distance, then the match, then one literal
    prefix = [rng.randrange(256) for _ in range(32768)]
    for n in (3, 4, 10, 11, 257, 258):
        for d in (1, 2, 3, 4, 7, 8, 63, 64, 65, 255, 256, 257, 32767, 32768):
            tk = prefix[:d] + [(n, d), 33]
            add("match %d at %d" % (n, d), fixed_stream(tk), tokens_text(tk))
    tk = prefix[:100] + [(258, 100)]
    add("match ends at ISIZE", fixed_stream(tk), tokens_text(tk))
    tk = prefix[:1000] + [(258, 1000)] * 250 + [(36, 7)]
    assert len(tokens_text(tk)) == 65536
    add("text of 65536", fixed_stream(tk), tokens_text(tk))
    add("extra subfield before BC", deflate(fq[:5000]), fq[:5000], extra=b"XY\x03\0abc")
    add("extra subfield after BC", deflate(fq[:5000]), fq[:5000], extra_after=b"ZZ\x00\0")
    out.append(("EOF block", EOF_BLOCK, b""))
    return out


def _retrailer(member, text):
    return member[:-8] + struct.pack("<II", zlib.crc32(text), len(text))


@functools.lru_cache(maxsize=None)
def damaged_fixtures():
    """[(name, member bytes, text_len the descriptor names, expected status)] -- every one a block zlib refuses"""
    fq = fastq_text(20000, seed=5)
    good = bgzf_member(deflate(fq), fq)
    out = []

    def add(name, member, status, text_len=len(fq)):
        out.append((name, member, text_len, status))

    def wrap(stream, text_len=100):  # a member around a (broken) stream, with a checksum that cannot be the cause
        return bgzf_member(stream, bytes(text_len))

    add("wrong magic", b"\x1f\x8c" + good[2:], HEADER)
    add("FLG without FEXTRA", good[:3] + b"\0" + good[4:], HEADER)
    add("XLEN beyond the block", good[:10] + struct.pack("<H", len(good)) + good[12:], HEADER)
    add("no BC subfield", good[:12] + b"BD" + good[14:], HEADER)
    add("BSIZE not length - 1", good[:16] + struct.pack("<H", len(good) - 2) + good[18:], HEADER)
    add("block type 3", wrap(b"\x07\x00"), DATA, 100)
    stored = deflate(fq[:100], 0)
    assert stored[0] == 1
    add("stored LEN / NLEN disagree", bgzf_member(stored[:3] + bytes([stored[3] ^ 1]) + stored[4:], fq[:100]), DATA, 100)
    add("stored LEN past the block", bgzf_member(struct.pack("<BHH", 1, 200, 200 ^ 0xFFFF) + fq[:100], fq[:100]), DATA, 100)
    # dynamic headers by hand: HLIT 257, HDIST 1, HCLEN 19
    w = BitWriter()
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4)
    for k in range(19):
        w.put(4, 3)  # 19 codes of 4 bits: 19/16 over-subscribes the code-length code
    add("over-subscribed code lengths", wrap(w.done() + bytes(8)), DATA, 100)
    w = BitWriter()
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4)
    for k in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]:
        w.put(1 if k in (16, 8) else 0, 3)  # two codes of one bit: 8 -> 0, 16 -> 1
    w.put(1, 1)  # symbol 16 first: repeat the previous length, and there is none
    add("repeat code without a previous length", wrap(w.done() + bytes(8)), DATA, 100)
    w = BitWriter()
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4)
    for k in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]:
        w.put(1 if k in (1, 2) else 0, 3)  # lengths 1 -> code 0, 2 -> code 1
    for k in range(258):
        w.put(0 if k < 3 else 1, 1)  # three literal/length codes of 1 bit: over-subscribed
    add("over-subscribed literal/length lengths", wrap(w.done() + bytes(8)), DATA, 100)
    w = BitWriter()
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4)
    for k in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]:
        w.put(2 if k in (0, 8) else 0, 3)  # two codes of two bits: half of the code-length code's space is unused
    add("incomplete code-length code", wrap(w.done() + bytes(8)), DATA, 100)
    w = BitWriter()
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4)
    for k in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]:
        w.put(1 if k in (0, 2) else 0, 3)  # lengths 0 -> code 0, 2 -> code 1
    for k in range(258):
        w.put(1 if k in (0, 256) else 0, 1)  # literal 0 and end-of-block, two bits each: an incomplete code of more than one bit
    add("incomplete literal/length code", wrap(w.done() + bytes(8)), DATA, 100)
    add("literal/length symbol 286", wrap(fixed_stream([65] * 100, raw_lit=286)), DATA, 100)
    add("distance symbol 30", wrap(fixed_stream([65] * 97, raw_dist=30)), DATA, 100)
    tk = [65] * 50
    add("distance beyond the text", bgzf_member(fixed_stream(tk + [(50, 51)]), bytes(100)), DATA, 100)
    for cut in (1, 2, 9):
        m = good[:-cut]
        add("cut short by %d" % cut, m[:16] + struct.pack("<H", len(m) - 1) + m[18:], DATA)
    add("ISIZE one less", good[:-4] + struct.pack("<I", len(fq) - 1), SIZE)
    add("ISIZE one more", good[:-4] + struct.pack("<I", len(fq) + 1), SIZE)
    add("text longer than the descriptor says", good, SIZE, len(fq) - 1)
    add("text shorter than the descriptor says", good, SIZE, len(fq) + 1)
    add("CRC bit flipped", good[:-8] + bytes([good[-8] ^ 4]) + good[-7:], CRC)
    return out


@functools.lru_cache(maxsize=None)
def flip_fixtures(n=200):
    """(text, [member with one byte flipped] * n): a level-6 member, flips at evenly spaced offsets"""
    fq = fastq_text(20000, seed=9)
    good = bgzf_member(deflate(fq), fq)
    rng = random.Random(1)
    out = []
    for k in range(n):
        at = k * len(good) // n
        out.append(good[:at] + bytes([good[at] ^ (1 << rng.randrange(8))]) + good[at + 1:])
    return fq, out


def zlib_verdict(member, text_len):
    """what zlib makes of a member whose text should be text_len bytes: the text, or None if it refuses it (an invalid
    stream, a wrong length or checksum, or a header that is not a BGZF block's)"""
    try:
        if len(member) < 28 or member[:4] != b"\x1f\x8b\x08\x04":
            return None
        xlen = struct.unpack_from("<H", member, 10)[0]
        if 12 + xlen + 8 > len(member):
            return None
        at, bsize = 0, None
        while at + 4 <= xlen:
            sid, slen = member[12 + at:14 + at], struct.unpack_from("<H", member, 14 + at)[0]
            if sid == b"BC" and slen == 2 and bsize is None:
                bsize = struct.unpack_from("<H", member, 16 + at)[0]
            at += 4 + slen
        if bsize is None or at != xlen or bsize + 1 != len(member):
            return None
        d = zlib.decompressobj(-15)
        text = d.decompress(member[12 + xlen:-8])
        if not d.eof:
            return None
        crc, isize = struct.unpack("<II", member[-8:])
        if len(text) != text_len or isize != text_len or zlib.crc32(text) != crc:
            return None
        return text
    except zlib.error:
        return None


def write_core_fixtures(path):
    """the file tests/cpp/inflate_core_check.cpp reads: every valid, damaged and flipped member with what to expect"""
    rows = [(m, t, OK) for _, m, t in valid_fixtures()]
    rows += [(m, bytes(n), st) for _, m, n, st in damaged_fixtures()]
    text, flips = flip_fixtures()
    rows += [(m, text, 255) for m in flips]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(rows)))
        for member, text, expect in rows:
            f.write(struct.pack("<IIB", len(member), len(text), expect) + member + text)
    return len(rows)
