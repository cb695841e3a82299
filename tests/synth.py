"""Small synthetic genomes/reads for parity tests (numpy, deterministic)."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
for a, b in zip(b"ACGTN", b"TGCAN"):
    COMP[a] = b


def repeat_rich_genome(path, seed=3, n_chroms=3, chrom_len=1_500_000, iupac=0):
    """Repeat families at low divergence, purine-only tracts, homopolymers and N
    runs (short ones get LCG-filled by the indexer, long ones are excluded): the
    inputs that drive bucket narrowing, full candidate heaps and tie handling."""
    rng = np.random.default_rng(seed)
    fams = [ACGT[rng.integers(0, 4, ln)] for ln in (320, 900, 2500)]
    with open(path, "wb") as f:
        for c in range(n_chroms):
            seq = ACGT[rng.integers(0, 4, chrom_len)].copy()
            for fam, copies, div in zip(fams, (600, 250, 80), (0.03, 0.02, 0.05)):
                for at in rng.integers(0, chrom_len - len(fam), copies):
                    piece = fam.copy()
                    m = rng.random(len(fam)) < div
                    piece[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
                    if rng.random() < 0.5:
                        piece = COMP[piece[::-1]]
                    seq[at:at + len(fam)] = piece
            for at in rng.integers(0, chrom_len - 500, 150):  # A/G-only and C/T-only tracts
                alpha = np.frombuffer(b"AG" if rng.random() < 0.5 else b"CT", dtype=np.uint8)
                seq[at:at + 400] = alpha[rng.integers(0, 2, 400)]
            for at in rng.integers(0, chrom_len - 300, 40):   # homopolymers / dinucleotide repeats
                motif = ACGT[rng.integers(0, 4, int(rng.integers(1, 3)))]
                seq[at:at + 200] = np.resize(motif, 200)
            if iupac:                                          # ambiguity codes: multi-bit genome nibbles
                at = rng.integers(0, chrom_len, iupac)
                seq[at] = np.frombuffer(b"RYMKSWBDHV", dtype=np.uint8)[rng.integers(0, 10, iupac)]
            seq[1000:1100] = ord("N")                          # short run (<=256): filled
            seq[chrom_len // 2: chrom_len // 2 + 3000] = ord("N")  # long run: excluded
            if c == 0:
                seq[:50] = ord("N")
            if c % 2 == 1:                                     # some soft-masked sequence
                seq[5000:9000] = np.char.lower(seq[5000:9000].view("S1")).view(np.uint8)
            f.write(b">chr%d some description\n" % (c + 1))
            f.write(b"\n".join(bytes(seq[i:i + 70]) for i in range(0, chrom_len, 70)) + b"\n")


def read_chroms(fasta):
    """the chromosomes of a FASTA as upper-case uint8 arrays"""
    return [np.frombuffer(rec.split(b"\n", 1)[1].replace(b"\n", b"").upper(), dtype=np.uint8)
            for rec in open(fasta, "rb").read().split(b">")[1:]]


def mutated_reads(fasta, n, L, seed, mut=0.02, bis=0.95, pbat_frac=0.0, n_frac=0.02):
    """Reads drawn from a FASTA with substitutions/indels and bisulfite conversion;
    a fraction carry N bases (leading/trailing/internal) and a few are too short."""
    rng = np.random.default_rng(seed)
    chroms = read_chroms(fasta)
    reads = []
    for _ in range(n):
        ch = chroms[int(rng.integers(0, len(chroms)))]
        ln = L if rng.random() > 0.05 else int(rng.integers(30, L))
        at = int(rng.integers(0, len(ch) - ln - 20))
        frag = ch[at:at + ln + 20].copy()
        if rng.random() < 0.5:
            frag = COMP[frag[::-1]]
        out = []
        i = 0
        while len(out) < ln and i < len(frag):
            r = rng.random()
            if r < mut / 3:
                out.append(ACGT[rng.integers(0, 4)]); i += 1
            elif r < 2 * mut / 3:
                out.append(ACGT[rng.integers(0, 4)])
            elif r < mut:
                i += 1
            else:
                out.append(frag[i]); i += 1
        s = np.array(out[:ln], dtype=np.uint8)
        ga = rng.random() < pbat_frac
        src, dst = (ord("G"), ord("A")) if ga else (ord("C"), ord("T"))
        conv = (s == src) & (rng.random(len(s)) < bis)
        s[conv] = dst
        if rng.random() < n_frac:
            k = int(rng.integers(1, 8))
            where = rng.random()
            if where < 0.33:
                s[:k] = ord("N")
            elif where < 0.66:
                s[-k:] = ord("N")
            else:
                j = int(rng.integers(0, len(s) - k)); s[j:j + k] = ord("N")
        reads.append(bytes(s))
    return reads


def trim_like_readloader(reads):
    """ReadLoader::load_reads trimming/skip rule (src/abismal.cpp:187-195) on raw sequences."""
    out = []
    for r in reads:
        if isinstance(r, bytes):
            r = r.decode()
        if sum(1 for c in r if c != "N") < 44:
            out.append("")
            continue
        r = r.rstrip("N")
        first = min(i for i in (r.find(b) for b in "ACGT") if i >= 0)
        out.append(r[first:])
    return out


def cut_pairs_ragged(r1, r2, rng, lo, hi):
    """Pairs generated at the batch's longest length, both ends of a pair truncated independently to lo..hi bases (uniform,
    both included); the last pair is kept whole so that the batch's longest end stays.  Apply trim_like_readloader afterwards."""
    out1 = [a[: int(rng.integers(lo, hi + 1))] for a in r1[:-1]] + [r1[-1]]
    out2 = [b[: int(rng.integers(lo, hi + 1))] for b in r2[:-1]] + [r2[-1]]
    return out1, out2


def cut_pairs_fixed(r1, r2, L1, L2):
    """Unequal ends: every end 1 truncated to L1 bases and every end 2 to L2.  Apply trim_like_readloader afterwards."""
    return [a[:L1] for a in r1], [b[:L2] for b in r2]


def pairs_at_n_runs(chroms, lengths, seed=4, mirrored=False, straddle=False, unmated=False):
    """Exact, fully converted pairs on a repeat_rich_genome: one end cut at distance 0..24 from the long N run in the middle
    of each chromosome, left of it and right of it, the other end 150-400 bases further out on the opposite strand.
    mirrored: also the same fragments read from the other strand, so that either end is the one at the run on both sides.
    straddle: also pairs whose ends lie either side of the short (LCG-filled) N run at 1000-1100, both strands.
    unmated: also pairs with one end at the long run and the other 50,000 bases further out, too far to be its mate: each
    end can only be reported on its own (fallback hits)."""
    r1, r2 = [], []
    rng = np.random.default_rng(seed)

    def add(fwd, rev):
        r1.append(bytes(fwd).decode().replace("C", "T"))
        r2.append(bytes(COMP[rev[::-1]]).decode().replace("G", "A"))
        if mirrored:
            r1.append(bytes(COMP[rev[::-1]]).decode().replace("C", "T"))
            r2.append(bytes(fwd).decode().replace("G", "A"))

    for ch in chroms:
        mid = len(ch) // 2
        for L in lengths:
            for k in range(25):
                gap = int(rng.integers(150, 400))
                a, b = ch[mid - L - k: mid - k], ch[mid - k - gap - L: mid - k - gap]         # left of the run
                c, d = ch[mid + 3000 + k: mid + 3000 + k + L], ch[mid + 3000 + k + gap: mid + 3000 + k + gap + L]  # right of it
                for fwd, rev in ((b, a), (c, d)):
                    add(fwd, rev)
            if unmated:
                for k in range(0, 25, 4):
                    add(ch[mid - k - 50_000 - L: mid - k - 50_000], ch[mid - L - k: mid - k])
                    add(ch[mid + 3000 + k: mid + 3000 + k + L], ch[mid + 3000 + k + 50_000: mid + 3000 + k + 50_000 + L])
            if straddle:
                for k in range(0, 25, 3):
                    add(ch[1000 - L - k: 1000 - k], ch[1100 + k: 1100 + k + L])
    return r1, r2


def mutated_pairs(fasta, n, L, seed, mut=0.02, bis=0.95, frag=(120, 600)):
    """Read pairs from random fragments: read 1 = fragment start, read 2 = revcomp of its end;
    conversion C->T on the fragment strand (so read 2 looks G->A), with mutations and some Ns."""
    rng = np.random.default_rng(seed)
    chroms = read_chroms(fasta)
    out1, out2 = [], []
    for _ in range(n):
        ch = chroms[int(rng.integers(0, len(chroms)))]
        fl = int(rng.integers(max(frag[0], L), frag[1]))
        at = int(rng.integers(0, len(ch) - fl))
        f = ch[at:at + fl].copy()
        if rng.random() < 0.5:
            f = COMP[f[::-1]]
        m = rng.random(fl) < mut
        f[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
        if rng.random() < 0.2:  # a small deletion or insertion
            j = int(rng.integers(10, fl - 10))
            f = np.concatenate([f[:j], f[j + 2:]]) if rng.random() < 0.5 else np.concatenate([f[:j], ACGT[rng.integers(0, 4, 2)], f[j:]])
        conv = (f == ord("C")) & (rng.random(len(f)) < bis)
        f[conv] = ord("T")
        a = f[:L].copy()
        b = COMP[f[::-1]][:L].copy()
        if rng.random() < 0.03:
            a[:3] = ord("N")
        if rng.random() < 0.03:
            b[-4:] = ord("N")
        if rng.random() < 0.02:
            a = a[:30]
        out1.append(bytes(a))
        out2.append(bytes(b))
    return out1, out2
