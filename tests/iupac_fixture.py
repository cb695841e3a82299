"""Genomes with IUPAC letters for tests/test_gpu_iupac_planes.py, and the rules the device structures follow, restated in
numpy from the FASTA alone: the genome's nibbles as the indexer lays them out, the chunks of the planes' map a blank or
multi-bit nibble flags, and full_compare's distances (src/abismal.cpp:1105-1122) beside the distance the bit planes give."""
import numpy as np

from tests import synth

PAD = 32767           # bases of N before the first and after the last chromosome (abm_index_build.cpp: load_fasta)
MAX_FILLED_RUN = 256  # N runs up to this length are filled with LCG bases, longer ones stay blank
CHUNK_BITS, REACH, BLOCK = 12, 512, 64  # abm_device.hpp: kPlaneChunkBits, kPlaneReach, kPlaneBlock

GENOME_CODE = np.zeros(256, dtype=np.uint8)  # dna_four_bit_encoding: N and everything else -> 0
for _c, _v in zip(b"ABCDGHKMRSTVWY", (1, 14, 2, 13, 4, 11, 12, 3, 5, 6, 8, 7, 9, 10)):
    GENOME_CODE[_c] = _v
POP4 = np.array([bin(k).count("1") for k in range(16)], dtype=np.int32)
MEMBERS = {"R": "AG", "Y": "CT", "M": "AC", "K": "GT", "S": "CG", "W": "AT", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG"}


def genome_nibbles(fasta):
    """(nibbles of the padded genome, start of every chromosome in it): pad, chromosomes, pad; short N runs filled from one
    LCG stream in genome order, long ones blank"""
    chroms = synth.read_chroms(fasta)
    text = np.concatenate([np.full(PAD, ord("N"), np.uint8)] + chroms + [np.full(PAD, ord("N"), np.uint8)])
    starts = np.cumsum([PAD] + [len(c) for c in chroms])[:-1]
    is_n = text == ord("N")
    edges = np.flatnonzero(np.diff(np.concatenate([[0], is_n.view(np.int8), [0]])))
    x = 1
    for a, b in zip(edges[::2], edges[1::2]):
        if b - a <= MAX_FILLED_RUN:
            for k in range(a, b):
                x = (1103515245 * x + 12345) & 0x7fffffff
                text[k] = b"ACGT"[x & 3]
    return GENOME_CODE[text], [int(s) for s in starts]


def plane_code(nib):
    """make_planes_kernel: low bit from bits 1|3 of the nibble, high bit from bits 2|3 (a one-hot nibble's bit index; 0 for a
    blank; for a multi-bit nibble whatever this gives, which nothing may trust)"""
    nib = nib.astype(np.uint32)
    return (((nib >> 1) | (nib >> 3)) & 1) | ((((nib >> 2) | (nib >> 3)) & 1) << 1)


def flagged_chunks(nib):
    """(chunks of the genome, chunks flagged): a 64-base block with a blank or multi-bit nibble flags every chunk from the
    one holding the position REACH bases before the block to the block's own"""
    n = len(nib)
    n_chunks = (n + (1 << CHUNK_BITS) - 1) >> CHUNK_BITS
    odd = (POP4[nib] != 1)
    blocks = np.flatnonzero(np.add.reduceat(odd.astype(np.int64), np.arange(0, n, BLOCK)) > 0)
    flag = np.zeros(n_chunks + 1, dtype=bool)
    for b in blocks:
        at = int(b) * BLOCK
        flag[max(at - REACH, 0) >> CHUNK_BITS: ((at + BLOCK - 1) >> CHUNK_BITS) + 1] = True
    return n_chunks, flag[:n_chunks]


def read_nibbles(seq, a_alphabet):
    """read_nibble (src/dna_four_bit_bisulfite.hpp:26-57): T-rich A 1, C 2, G 4, T 10; A-rich A 5, C 2, G 4, T 8"""
    t = np.zeros(256, dtype=np.uint8)
    for c, v in zip(b"ACGT", (5, 2, 4, 8) if a_alphabet else (1, 2, 4, 10)):
        t[c] = v
    return t[np.frombuffer(seq.encode() if isinstance(seq, str) else seq, dtype=np.uint8)]


def revcomp(seq):
    return bytes(synth.COMP[np.frombuffer(seq.encode(), dtype=np.uint8)[::-1]]).decode()


def distances(nib, pos, seq, rc=False, g_to_a=False):
    """full_compare of read `seq` (as handed to the mapper) at genome position pos in orientation (rc, alphabet): (d, dmax,
    plane distance).  d: 16 - popcount(read word & genome word) summed over the read's words, the last one padded with 0xF;
    dmax: the largest prefix sum (never below 0); plane distance: read bases whose nibble lacks the bit of the genome base's
    plane code."""
    q = read_nibbles(revcomp(seq) if rc else seq, g_to_a)
    L = len(q)
    W = (L + 15) // 16
    qp = np.full(16 * W, 15, dtype=np.uint8)
    qp[:L] = q
    g = np.zeros(16 * W, dtype=np.uint8)
    have = nib[pos:pos + 16 * W]
    g[:len(have)] = have
    share = 16 - POP4[qp & g].reshape(W, 16).sum(axis=1)
    prefix = np.cumsum(share)
    plane = int((((q.astype(np.uint32) >> plane_code(g[:L])) & 1) == 0).sum())
    return int(prefix[-1]), max(0, int(prefix.max())), plane


def _convert(seq):
    return seq.replace("C", "T")


def hand_built_genome(path, seed=7):
    """One chromosome of 160 kbp, no N, with IUPAC letters where scattering them at random will not put them.  Returns the
    planted single-end reads (mode 0, both lengths) as a list of dicts {seq, L, at (offset of the window's first base in the
    chromosome), kind, rc}; kinds:
      first / last / before / after / near   one letter on the window's first base, its last, the base before it, the base after
                                    it, or 7 ... 183 bases past its start -- among them the last base a record's stretch
                                    covers and the first beyond, whatever seed offset the index holds an entry for
      chunk        a letter on a chunk's first base, windows starting 1 ... 600 bases before it in the chunk before
      matches      (a) 55 % of the window is K in the genome and G in the read: distance 0-2, plane distance above 0.4 L
      prefix       (b) the read's first three (four) words mismatch everywhere and the rest is T on Y, a share of -1 each: the
                   prefix sum passes 0.4 L, the total ends within L / 10
      clean        windows in the half of the chromosome that holds no letter"""
    rng = np.random.default_rng(seed)
    n = 160_000
    seq = synth.ACGT[rng.integers(0, 4, n)].copy()
    letters = "RYMKSWBDHV"
    planted = []

    def put(at, letter):
        seq[at] = ord(letter)

    def cut(w, L, kind, rc=False, member=True):
        s = bytes(seq[w:w + L]).decode()
        out = []
        for k, c in enumerate(s):
            if c in MEMBERS:
                ok = MEMBERS[c]
                c = ok[(w + k) % len(ok)] if member else next(x for x in "ACGT" if x not in ok)
            out.append(c)
        s = "".join(out)
        s = _convert(revcomp(s) if rc else s)
        planted.append(dict(seq=s, L=L, at=w, kind=kind, rc=rc))

    # isolated letters, one per site
    at = 2_000
    k = 0
    for L in (100, 150):
        for rep in range(6):
            site = at
            put(site, letters[k % 10])
            for delta, kind in ((0, "first"), (L - 1, "last"), (-1, "before"), (L, "after"), (L + 7, "near"), (L + 8, "near"), (107, "near"),
                                (108, "near"), (139, "near"), (140, "near"), (171, "near"), (172, "near"), (182, "near"), (183, "near")):
                cut(site - delta, L, kind, rc=bool((k + delta) & 1), member=bool((k + delta) & 2))
            at += 900
            k += 1
    # chunk boundaries: absolute position c << 12 is offset (c << 12) - PAD
    for c in (12, 15, 18):
        site = (c << CHUNK_BITS) - PAD
        assert site - (1 << CHUNK_BITS) > at - 900, "the chunk before the site holds no letter of its own"
        put(site, letters[c % 10])
        for L in (100, 150):
            for delta in (1, 64, 100, 300, 448, 511, 512, 513, 600):
                cut(site - delta, L, "chunk", rc=bool(delta & 1))
    # (a) letters that match where their plane code does not
    a0 = 50_000
    span = 1200
    stretch = np.where(rng.random(span) < 0.55, ord("G"), np.frombuffer(b"ACT", dtype=np.uint8)[rng.integers(0, 3, span)]).astype(np.uint8)
    seq[a0:a0 + span] = stretch
    seq[a0:a0 + span][stretch == ord("G")] = ord("K")
    for L in (100, 150):
        for w in range(a0, a0 + span - L, 31):
            s = bytes(seq[w:w + L]).decode().replace("K", "G")
            if (w // 31) % 3 == 0:  # (some with two substitutions)
                s = s[:20] + ("A" if s[20] != "A" else "G") + s[21:60] + ("A" if s[60] != "A" else "G") + s[61:]
            planted.append(dict(seq=_convert(s), L=L, at=w, kind="matches", rc=False))
    # (b) prefix sums above the cutoff, totals within it
    b0 = 56_000
    wrong = {ord("A"): "G", ord("C"): "A", ord("G"): "A", ord("T"): "A"}
    for L, p1, n_y in ((100, 48, 42), (150, 64, 58)):
        for rep in range(30):
            w = b0
            p2 = L - p1
            tail = np.frombuffer(b"AG", dtype=np.uint8)[rng.integers(0, 2, p2)].copy()
            tail[rng.permutation(p2)[:n_y]] = ord("Y")
            seq[w + p1:w + L] = tail
            s = "".join(wrong[c] for c in seq[w:w + p1]) + bytes(tail).decode().replace("Y", "T")
            planted.append(dict(seq=s, L=L, at=w, kind="prefix", rc=False))
            b0 += L + 250
    assert b0 < 80_000
    # the clean half
    for L in (100, 150):
        for w in range(90_000, 150_000, 331):
            cut(w, L, "clean", rc=bool(w & 1))
    assert not any(chr(c) in MEMBERS for c in seq[84_000:])
    with open(path, "wb") as f:
        f.write(b">hand built\n")
        f.write(b"\n".join(bytes(seq[i:i + 70]) for i in range(0, n, 70)) + b"\n")
    return planted


def mates_for(fasta, planted, gap=230):
    """pairs from the planted reads: end 1 is the planted read, end 2 the reverse complement of the stretch `gap` bases past
    the window's end, fully converted as an end 2 is (G -> A); letters in it replaced by a member"""
    ch = synth.read_chroms(fasta)[0]
    r1, r2 = [], []
    for p in planted:
        if p["rc"]:
            continue
        w = p["at"] + p["L"] + gap
        s = "".join(MEMBERS[c][0] if c in MEMBERS else c for c in bytes(ch[w:w + p["L"]]).decode())
        r1.append(p["seq"])
        r2.append(revcomp(s).replace("G", "A"))
    return r1, r2
