"""The texts the BGZF deflate tests encode (CPU and GPU files share them), and what every encoding of them must satisfy."""
import functools
import gzip
import random
import struct

import numpy as np

from tests import bam_format as B
from tests import deflate_tools as D

BLOCK = 0xff00
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17]
BLOCK_BYTES = [0, 7919]
FULL = LENGTHS[-1]


@functools.lru_cache(maxsize=None)
def bam_stream(n_bytes, seed=5):
    """a BAM-like record stream, as `map -B` hands it to the deflater: 100-base reads along one chromosome, a quarter on
    the reverse strand, names that count up, absent qualities"""
    rng, out, k, pos = random.Random(seed), bytearray(), 0, 1000
    while len(out) < n_bytes:
        seq = "".join(rng.choice("ACGT") for _ in range(100))
        pos += rng.randrange(1, 40)
        rc = rng.random() < 0.25
        cig = [100 << 4] if rng.random() < 0.9 else [(60 << 4), (1 << 4) | 1, (39 << 4)]
        pc = B.piece(0x10 if rc else 0, 0, pos, cig, "*", 0, 0, seq, rc, rng.randrange(4), "T" if rng.random() < 0.5 else "A")
        out += B.assemble("SRR0000001.%d" % k, pc)
        k += 1
    return bytes(out[:n_bytes])


@functools.lru_cache(maxsize=None)
def cases():
    """{name: FULL bytes of text}; a test takes prefixes of them"""
    rng = random.Random(3)
    piece = bytes(rng.getrandbits(8) for _ in range(40000))
    period = bytes(rng.getrandbits(8) for _ in range(7))
    out = {
        "zeros": bytes(FULL),
        "ff": b"\xff" * FULL,
        "text": b"".join(b"@read%d\nACGTTGCA%s\n+\nIIIIIIII\n" % (k, b"ACGT"[k % 4:k % 4 + 1] * (k % 50)) for k in range(20000))[:FULL],
        "fastq": D.fastq_text(FULL),
        "random": bytes(rng.getrandbits(8) for _ in range(FULL)),
        "high": bytes(144 + rng.randrange(112) for _ in range(FULL)),
        "period7": (period * (FULL // 7 + 1))[:FULL],
        "four times 40000": (piece * 5)[:FULL],
        "bam": bam_stream(FULL),
    }
    assert all(len(v) == FULL for v in out.values())
    return out


def every_text():
    """[(id, text, block_bytes)]: every case at every length and both block sizes (a length is taken once where the
    prefixes of two cases are the same text: the empty one)"""
    out = []
    for name, data in cases().items():
        for n in LENGTHS:
            if n == 0 and name != "zeros":
                continue
            for bb in BLOCK_BYTES:
                out.append(("%s[:%d] / %d" % (name, n, bb), data[:n], bb))
    return out


def window_edge_texts():
    """[(id, text, block_bytes)], tokens_text-style: eight bytes found nowhere else, a run of one letter -- which the
    encoder takes as matches at distance 1 and which leaves the table's entry for the eight bytes alone -- and, exactly
    32768 / 32769 bytes after the text's start, a copy of its first 200 bytes: a match the encoder has to take whole, and
    one it must not take.  Then a match that ends on the block's last byte, and one that crosses the end of a round of 64."""
    rng = random.Random(9)
    out = []
    for d in (32768, 32769):
        tk = list(range(1, 9)) + [97] * (d - 8) + [(200, d), 33]
        out.append(("match 200 at %d" % d, D.tokens_text(tk), 0))
    tk = [rng.randrange(97, 123) for _ in range(100)] + [(258, 100)]
    out.append(("match ends the block", D.tokens_text(tk), 0))
    tk = [rng.randrange(97, 123) for _ in range(60)] + [(100, 60), 33, 34]
    out.append(("match crosses a round's end", D.tokens_text(tk), 0))
    return out


def members_of(out, blocks):
    return [out[int(b["at"]):int(b["at"]) + int(b["len"])] for b in blocks]


def check_members(data, block_bytes, out, blocks, bound):
    """what holds for every encoding: framing, tiling, zlib's verdict on every member (CRC-32 and ISIZE), the bound"""
    bb = block_bytes or BLOCK
    assert len(blocks) == -(-len(data) // bb)
    assert gzip.decompress(out + D.EOF_BLOCK) == data
    at = t = 0
    for b, m in zip(blocks, members_of(out, blocks)):
        assert (int(b["at"]), int(b["text_at"])) == (at, t)
        assert int(b["text_len"]) == min(bb, len(data) - t)
        assert len(m) == int(b["len"]) <= 65536 and len(m) <= int(b["text_len"]) + 31
        assert m[:4] == b"\x1f\x8b\x08\x04" and m[12:16] == b"BC\x02\0"
        assert struct.unpack_from("<H", m, 16)[0] + 1 == len(m)
        assert D.zlib_verdict(m, int(b["text_len"])) == data[t:t + int(b["text_len"])]
        at, t = at + len(m), t + int(b["text_len"])
    assert at == len(out) and t == len(data)
    assert len(out) <= bound


def walked(out, blocks):
    """D.walk's tallies of every member's stream"""
    return [D.walk(m[18:-8])[1] for m in members_of(out, blocks)]


def blocks_equal(a, b):
    return len(a) == len(b) and bool(np.array_equal(a, b))
