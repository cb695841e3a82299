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


# ---- one satellite family of tens of thousands of copies: paired-end candidate sets at their limit of 32768 entries -----
def satellite_genome(path, copies, unit_len, divergence, lead, seed, iupac=0):
    """One chromosome of random sequence without N: `lead` bases, then `copies` copies of one random unit of unit_len
    bases, evenly spaced at unit_len + 20, each with its own substitutions at `divergence`, all on one strand, then `lead`
    bases more.  iupac: that many ambiguity letters in the two flanks, none inside the family (the genome then has no bit
    planes).  With max_candidates raised to 30000 a read cut from a copy finds every copy: its candidate set fills.
    The mating reaches back max_frag bases from a hit: pairs_on_satellite asserts that the first copy lies further in than
    that (oracle/README.md, "Hits near the genome's first base").  Returns the layout pairs_on_satellite and
    reads_on_satellite cut from."""
    rng = np.random.default_rng(seed)
    step = unit_len + 20
    n = 2 * lead + copies * step
    seq = ACGT[rng.integers(0, 4, n)].copy()
    unit = ACGT[rng.integers(0, 4, unit_len)]
    starts = lead + step * np.arange(copies)
    fam = np.tile(unit, (copies, 1))
    m = rng.random(fam.shape) < divergence
    fam[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
    for at, piece in zip(starts, fam):
        seq[at:at + unit_len] = piece
    if iupac:
        at = np.concatenate([rng.integers(0, lead - 1000, iupac // 2), n - lead + 1000 + rng.integers(0, lead - 1000, iupac - iupac // 2)])
        seq[at] = np.frombuffer(b"RYMKSWBDHV", dtype=np.uint8)[rng.integers(0, 10, iupac)]
    assert not (seq == ord("N")).any()
    with open(path, "wb") as f:
        f.write(b">sat\n" + b"\n".join(bytes(seq[i:i + 70]) for i in range(0, n, 70)) + b"\n")
    return {"lead": lead, "copies": copies, "unit_len": unit_len, "step": step}


def _planted(s, rng, subs, indel):
    """up to `subs` substitutions, and with indel one base dropped or one inserted, away from the ends; length kept"""
    s = s.copy()
    L = len(s)
    at = rng.integers(0, L, int(rng.integers(1, subs + 1))) if subs else []
    for j in at:
        s[j] = ACGT[(int(np.searchsorted(ACGT, s[j])) + int(rng.integers(1, 4))) % 4]
    if indel:
        j = int(rng.integers(25, L - 25))
        s = np.concatenate([s[:j], s[j + 1:], s[-1:]]) if rng.random() < 0.5 else np.concatenate([s[:j], ACGT[rng.integers(0, 4, 1)], s[j:-1]])
    return s


def pairs_on_satellite(lay, fasta, n, L, seed, max_frag=3000, planted=0.5, indels=0.25, same_strand=0.125):
    """n fully converted pairs of 2 x L from a satellite_genome: the fragment is one copy (unit_len bases, L <= unit_len),
    end 1 its first L bases C -> T, end 2 the reverse complement of its last L bases (so G -> A).  A share `planted` of
    the pairs carries 1-3 substitutions per end, a share `indels` of those a one-base insertion or deletion per end as well
    (winners that need the DP and a gapped traceback).  A share `same_strand` has end 2 NOT reverse-complemented: its ends
    find their copies in different orientation calls, so it can only be reported end by end (fallback hits only), from
    full sets.  max_frag: the largest fragment limit the pairs will be mapped with -- the first copy must lie further in."""
    assert lay["lead"] > max_frag + L, "the mating would reach the genome's first base: raise lead"
    assert L <= lay["unit_len"]
    rng = np.random.default_rng(seed)
    ch = read_chroms(fasta)[0]
    r1, r2 = [], []
    for k in rng.choice(lay["copies"], n, replace=False):
        at = lay["lead"] + int(k) * lay["step"]
        f = ch[at:at + lay["unit_len"]]
        a, b = f[:L], f[-L:]
        if rng.random() < planted:
            ind = rng.random() < indels
            a, b = _planted(a, rng, 3, ind), _planted(b, rng, 3, ind)
        a = a.copy()
        a[a == ord("C")] = ord("T")
        if rng.random() < same_strand:
            b = b.copy()
            b[b == ord("G")] = ord("A")
        else:
            b = COMP[b[::-1]]
            b[b == ord("G")] = ord("A")
        r1.append(bytes(a).decode())
        r2.append(bytes(b).decode())
    return r1, r2


def reads_on_satellite(lay, fasta, n, L, seed, ragged=0.3, planted=0.5):
    """n single-end reads from a satellite_genome, fully C -> T converted, every other one from the other strand; a share
    `ragged` is cut to 47 ... L - 1 bases, a share `planted` carries 1-3 substitutions"""
    rng = np.random.default_rng(seed)
    ch = read_chroms(fasta)[0]
    out = []
    for i, k in enumerate(rng.choice(lay["copies"], n, replace=False)):
        at = lay["lead"] + int(k) * lay["step"] + int(rng.integers(0, lay["unit_len"] - L + 1))
        s = ch[at:at + L]
        if rng.random() < planted:
            s = _planted(s, rng, 3, False)
        if i % 2:
            s = COMP[s[::-1]]
        if rng.random() < ragged:
            s = s[: int(rng.integers(47, L))]
        s = s.copy()
        s[s == ord("C")] = ord("T")
        out.append(bytes(s).decode())
    return out


# ---- repeat copies cut short by N runs: bucket narrowing where the probed letters are blank -----------------------------
def repeats_against_n_runs(path, seed=17, n_chroms=2, chrom_len=130_000, n_full=160, n_trunc=40, fwd_frac=0.85,
                           div=(0.01, 0.02), fam_len=300, run_len=300, unit=10):
    """One repeat family of fam_len bases in n_full whole copies at 1-2 % divergence, mostly on one strand so that a
    seed inside the family finds a bucket of more than 100 entries; n_trunc copies cut short -- the first t bases of
    the oriented family, t spread over 30 ... fam_len - 10, then run_len N (more than 256: the indexer leaves the run
    blank) -- so that the index entry o bases into such a copy has blank letters from depth t - o on and lies in the
    bucket of the whole copies' entries at family offset o; one whole copy on the genome's last bases (its entries run
    into the end padding); and one whole copy with 40 N inside (a short run, which the indexer fills: the control).
    Returns the layout the read generators below cut from: {"fam", "full": [(chrom, at, strand)], "trunc": [(chrom, at,
    strand, t)], "last": (chrom, at), "filled": (chrom, at)}; strand 1 = the family's reverse complement."""
    rng = np.random.default_rng(seed)
    fam = _n_run_family(rng, fam_len, unit)
    slot = 2 * fam_len + run_len + 50  # a copy, its run and background between neighbours
    per = (chrom_len - 2 * slot) // slot
    assert n_chroms * per >= n_full + n_trunc + 1, "not enough room for the copies"
    slots = [(c, slot + k * slot) for c in range(n_chroms) for k in range(per)]
    order = rng.permutation(len(slots))
    seqs = [ACGT[rng.integers(0, 4, chrom_len)].copy() for _ in range(n_chroms)]

    def oriented(strand):
        return COMP[fam[::-1]] if strand else fam

    def diverged(piece):
        piece = piece.copy()
        m = rng.random(len(piece)) < rng.uniform(*div)
        piece[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
        return piece

    lay = {"fam": fam, "full": [], "trunc": [], "fam_len": fam_len, "run_len": run_len}
    k = 0
    for _ in range(n_full):
        c, at = slots[order[k]]; k += 1
        strand = int(rng.random() >= fwd_frac)
        seqs[c][at:at + fam_len] = diverged(oriented(strand))
        lay["full"].append((c, at, strand))
    for j in range(n_trunc):
        c, at = slots[order[k]]; k += 1
        strand = int(rng.random() >= fwd_frac)
        t = 30 + (j * (fam_len - 40)) // max(1, n_trunc - 1)
        seqs[c][at:at + t] = diverged(oriented(strand))[:t]
        seqs[c][at + t:at + t + run_len] = ord("N")
        lay["trunc"].append((c, at, strand, t))
    c, at = slots[order[k]]
    piece = diverged(fam)
    piece[120:160] = ord("N")
    seqs[c][at:at + fam_len] = piece
    lay["filled"] = (c, at)
    seqs[-1][chrom_len - fam_len:] = diverged(fam)
    lay["last"] = (n_chroms - 1, chrom_len - fam_len)
    with open(path, "wb") as f:
        for c, seq in enumerate(seqs):
            f.write(b">chr%d\n" % (c + 1))
            f.write(b"\n".join(bytes(seq[i:i + 70]) for i in range(0, chrom_len, 70)) + b"\n")
    return lay


def _n_run_family(rng, fam_len, unit):
    """The family: its first half repeats one random unit, its second half one purine-only unit.  The indexer keeps one
    position in twenty, each copy its own, so a family without inner structure would spread 160 copies over buckets of a
    dozen entries; a repeated unit brings every kept position of every copy into one of `unit` buckets per table.  And a
    position goes to the 2-letter table OR to the 3-letter ones, whichever buckets are emptier: the purine half (one 2-letter
    bucket for all of it) is what puts entries, whole and cut short, into the 3-letter tables."""
    half = fam_len // 2
    a = np.resize(ACGT[rng.integers(0, 4, unit)], half)
    b = np.resize(np.frombuffer(b"AG", dtype=np.uint8)[rng.integers(0, 2, unit)], fam_len - half)
    return np.concatenate([a, b])


def _n_run_fragments(lay, chroms, L, rng, per_copy, frag):
    """Fragments (top-strand sequence as uint8 arrays) whose FIRST L bases are the read the issue is about:
    kind a: cut from a whole copy so that the seeds of the read's first half fall on the family offsets 25 ... 45 bases before
            the place where a cut-short copy of the same orientation ends (their buckets hold that copy's blank-tailed entries);
    kind b: cut from a cut-short copy, the read ending on the last base before the run (returned reversed: see below);
    kind c: starting inside a cut-short copy and continuing past the cut with the family's sequence, as the run were not there.
    Every fragment is (kind, array, flip) with the read of interest = array[:L] if not flip, else the last L bases."""
    fam_len = lay["fam_len"]
    out = []
    by_strand = {s: [x for x in lay["full"] if x[2] == s] for s in (0, 1)}
    for (c, at, strand, t) in lay["trunc"]:
        fam = COMP[lay["fam"][::-1]] if strand else lay["fam"]
        for _ in range(per_copy):
            flen = int(rng.integers(max(frag[0], L), frag[1]))
            # a: a whole copy of the same orientation
            cc, fat, _s = by_strand[strand][int(rng.integers(0, len(by_strand[strand])))] if by_strand[strand] else lay["full"][0]
            lo, hi = max(0, t - 45 - L // 2 + 1), max(0, min(fam_len - L, t - 25))
            s = int(rng.integers(min(lo, hi), hi + 1))
            out.append(("a", chroms[cc][fat + s: fat + s + flen].copy(), False))
            # b: ends on the last base before the run
            end = at + t
            out.append(("b", chroms[c][end - flen: end].copy(), True))
            # c: continues past the cut with family sequence (and background after the family's end)
            k = int(rng.integers(25, max(26, min(t, L - 20))))
            piece = np.concatenate([chroms[c][at + t - k: at + t], fam[t:]])[:L]
            if len(piece) < L:
                piece = np.concatenate([piece, ACGT[rng.integers(0, 4, L - len(piece))]])
            up = chroms[c][at + t - k - (flen - L): at + t - k]
            out.append(("c", np.concatenate([up, piece]), True))
    # the copy on the genome's last bases, and the copy with the filled run
    c, at = lay["last"]
    for _ in range(2 * per_copy):
        flen = int(rng.integers(max(frag[0], L), frag[1]))
        out.append(("b", chroms[c][len(chroms[c]) - flen:].copy(), True))
    c, at = lay["filled"]
    for _ in range(2 * per_copy):
        flen = int(rng.integers(max(frag[0], L), frag[1]))
        s = int(rng.integers(0, 100))
        out.append(("a", chroms[c][at + s: at + s + flen].copy(), False))
    return out


def _bisulfite(s, rng, ga, bis):
    src, dst = (ord("G"), ord("A")) if ga else (ord("C"), ord("T"))
    s = s.copy()
    s[(s == src) & (rng.random(len(s)) < bis)] = dst
    return s


def _sprinkle(s, rng, mut):
    s = s.copy()
    m = (rng.random(len(s)) < mut) & (s != ord("N"))
    s[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
    return s


def reads_against_n_runs(lay, fasta, L, seed, mode=0, per_copy=2, background=60, mut=0.005, bis=0.95):
    """Single-end reads for repeats_against_n_runs (kinds a, b, c of _n_run_fragments, either strand, plus random background);
    mode 0: C->T converted, 1: G->A, 2: half and half.  Apply trim_like_readloader afterwards."""
    rng = np.random.default_rng(seed)
    chroms = read_chroms(fasta)
    reads = []
    for kind, f, flip in _n_run_fragments(lay, chroms, L, rng, per_copy, (L, L + 1)):
        s = f[-L:] if flip else f[:L]
        s = _sprinkle(s, rng, mut)
        if rng.random() < 0.5:
            s = COMP[s[::-1]]
        ga = mode == 1 or (mode == 2 and rng.random() < 0.5)
        reads.append(bytes(_bisulfite(s, rng, ga, bis)))
    pb = {0: 0.0, 1: 1.0, 2: 0.5}[mode]
    return reads + mutated_reads(fasta, background, L, seed + 1, pbat_frac=pb)


def pairs_against_n_runs(lay, fasta, L, seed, per_copy=2, background=100, unmated=12, mut=0.005, bis=0.95, frag=(160, 420)):
    """Pairs for repeats_against_n_runs: one end is a read of kind a, b or c, its mate comes from the same fragment's other
    end; `unmated` pairs have their ends on different chromosomes (fallback hits only); plus random background.  Conversion
    as mutated_pairs: C->T on the fragment's strand.  Apply trim_like_readloader afterwards."""
    rng = np.random.default_rng(seed)
    chroms = read_chroms(fasta)
    r1, r2 = [], []

    def add(f):
        f = _bisulfite(_sprinkle(f, rng, mut), rng, False, bis)
        r1.append(bytes(f[:L]))
        r2.append(bytes(COMP[f[::-1]][:L]))

    frags = _n_run_fragments(lay, chroms, L, rng, per_copy, (max(frag[0], L + 20), frag[1]))
    for kind, f, flip in frags:
        add(COMP[f[::-1]] if rng.random() < 0.5 else f)
    for k in range(unmated):  # a read of interest with an end from elsewhere
        kind, f, flip = frags[int(rng.integers(0, len(frags)))]
        s = f[-L:] if flip else f[:L]
        ch = chroms[k % len(chroms)]
        at = (2 * lay["fam_len"] + lay["run_len"] + 50) * (3 + k) - 320  # (background between two copies' slots)
        other = ch[at:at + L]
        r1.append(bytes(_bisulfite(s, rng, False, bis)))
        r2.append(bytes(_bisulfite(other, rng, True, bis)))
    b1, b2 = mutated_pairs(fasta, background, L, seed + 1, frag=(max(120, L), 600))
    return r1 + b1, r2 + b2
