"""The edge matrix recorded from the reference mapper itself.

oracle/_ref/abismal_ref (and abismal_ref_short, its window-12 build) are the reference's own `map` and `idx`, compiled
from its sources with the stand-in headers of oracle/ref_shims/.  This module holds the table of cases, the builders of
their inputs (deterministic, on top of tests/synth.py; nothing but tests/golden/tRex1.fa is read), the helpers that run one
case through any of the three command lines -- reference, oracle, product -- and the recorder:

    python -m tests.reference_edges --record

runs every case through the reference at its default -t 1 and writes tests/golden/reference_edges.json: per case its flags,
the md5 of every input, the number of records, the md5 of the SAM without its @PG line (the one line that carries the
command line) and the md5 of the statistics file; and the md5 of every index file.  tests/test_reference_binary.py (CPU:
oracle and reference against the manifest) and tests/test_gpu_reference_edges.py (GPU: the product's command line against
the manifest) read it.  The manifest is what the reference answered: it is recorded, never edited."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MANIFEST = os.path.join(GOLD, "reference_edges.json")
REF = os.path.join(ROOT, "oracle", "_ref", "abismal_ref")
REF_SHORT = os.path.join(ROOT, "oracle", "_ref", "abismal_ref_short")
ORACLE_CLI = os.path.join(ROOT, "oracle", "_build", "abismal_oracle")
PRODUCT_CLI = os.path.join(ROOT, "abismal_amd", "abismal-amd")

# index name -> (genome file, window, targets file or None)
INDEXES = {
    "rep": ("rep.fa", 20, None),              # 2 x 400 kbp, repeat-rich, IUPAC letters, short and long N runs
    "rep_w12": ("rep.fa", 12, None),          # the same genome under the reference's --enable-short build
    "rep_targets": ("rep.fa", 20, "targets.bed"),
    "plain": ("plain.fa", 20, None),          # the genome of test_windows_that_reach_into_an_n_run: no IUPAC letters
    "trex": ("tRex1.fa", 20, None),           # the reference's own fixture, for the long reads
    "sat": ("sat.fa", 20, None),              # one family of 30000 copies at 2.5 % divergence (synth.satellite_genome)
    "sat_exact": ("sat_exact.fa", 20, None),  # the same family without divergence
}

SE, SE12, SET = ["se.fq"], ["se_w12.fq"], ["se_targets.fq"]
PE, PBAT, MIX = ["pe_1.fq", "pe_2.fq"], ["pbat_1.fq", "pbat_2.fq"], ["mix_1.fq", "mix_2.fq"]
SAT, SAT_EXACT = ["sat_1.fq", "sat_2.fq"], ["sat_exact_1.fq", "sat_exact_2.fq"]
# the satellite cases' own floor: 64 pairs and 256 reads go in, every one of them cut from the family; at least 64 records
# must come out (and, with -a on the family without divergence, at least 64 of them flagged secondary)
SAT_PAIRS, SAT_READS, SAT_MIN_RECORDS = 64, 256, 64
SAT_FAMILY = dict(copies=30000, unit_len=200, lead=41000, seed=5)  # (lead: beyond -L 40000 plus an end, see synth.pairs_on_satellite)


def _case(name, index, reads, flags=(), **more):
    return dict(name=name, index=index, reads=list(reads), flags=list(flags), **more)


CASES = [
    # single-end on the repeat-rich IUPAC genome: ragged reads, 40 % of them 44-46 bases, half of them G->A converted
    _case("se_default", "rep", SE),
    _case("se_A", "rep", SE, ["-A"]),
    _case("se_R", "rep", SE, ["-R"]),
    _case("se_P", "rep", SE, ["-P"]),
    _case("se_a", "rep", SE, ["-a"]),
    _case("se_c5", "rep", SE, ["-c", "5"]),
    _case("se_c1_a", "rep", SE, ["-c", "1", "-a"]),
    _case("se_R_a_c3", "rep", SE, ["-R", "-a", "-c", "3"]),
    _case("se_m0.2", "rep", SE, ["-m", "0.2"]),
    _case("se_m0.02", "rep", SE, ["-m", "0.02"]),
    _case("se_j", "rep", SE, ["-j"]),
    # paired-end on the same genome: ends of 40-110 bases, cut independently
    _case("pe_default", "rep", PE),
    _case("pe_P_pbat", "rep", PBAT, ["-P"]),           # true PBAT pairs: the ends swapped
    _case("pe_R_mix", "rep", MIX, ["-R"]),             # every other pair swapped
    _case("pe_a", "rep", PE, ["-a"]),
    _case("pe_c5", "rep", PE, ["-c", "5"]),
    _case("pe_l150_L300", "rep", PE, ["-l", "150", "-L", "300"]),
    _case("pe_R_a_c2", "rep", MIX, ["-R", "-a", "-c", "2"]),
    _case("pe_m0.2_L200", "rep", PE, ["-m", "0.2", "-L", "200"]),
    # reads and pairs cut at the edges of N runs
    _case("nrun_se", "plain", ["nrun.fq"]),
    _case("nrun_pe", "plain", ["nrun_1.fq", "nrun_2.fq"]),
    # long reads on tRex1, each set among ordinary reads
    _case("long_se", "trex", ["long.fq"], long_reads=True),
    _case("long_se_beyond_16383", "trex", ["longer.fq"], long_reads=True),
    _case("long_pe_L40000", "trex", ["long_1.fq", "long_2.fq"], ["-L", "40000"], long_reads=True),
    _case("too_long_se", "trex", ["too_long.fq"], refused=True),  # a read of 32,767 bases: the reference exits with an error
    # window 12 (abismal_ref_short): reads of 36-46 bases among ordinary ones
    _case("w12_se", "rep_w12", SE12),
    _case("w12_pe", "rep_w12", ["pe_w12_1.fq", "pe_w12_2.fq"]),
    # idx -A targets: reads from inside, across and outside the regions
    _case("targets_se", "rep_targets", SET),
    _case("targets_pe", "rep_targets", ["pe_targets_1.fq", "pe_targets_2.fq"]),
    # -c 30000 on the satellite family: paired-end candidate sets at their limit of 32768 entries (the fixture of
    # tests/test_gpu_pe_full_sets.py: 64 pairs of 2 x 100, 256 reads), mating windows of about 180 partners with -L 40000,
    # and the family without divergence, whose full sets at cutoff 0 make the reference skip the mating
    _case("pe_c30000", "sat", SAT, ["-c", "30000"], min_records=SAT_MIN_RECORDS),
    _case("pe_c30000_L40000", "sat", SAT, ["-c", "30000", "-L", "40000"], min_records=SAT_MIN_RECORDS),
    _case("pe_R_c30000", "sat", ["sat_mix_1.fq", "sat_mix_2.fq"], ["-R", "-c", "30000"], min_records=SAT_MIN_RECORDS),  # every other pair swapped
    # (without -a the family without divergence gives no record at all -- every end is ambiguous: the statistics file is the answer)
    _case("pe_c30000_exact", "sat_exact", SAT_EXACT, ["-c", "30000"], min_records=0),
    _case("pe_a_c30000_exact", "sat_exact", SAT_EXACT, ["-a", "-c", "30000"], min_records=SAT_MIN_RECORDS, min_secondary=SAT_MIN_RECORDS),
    _case("se_c30000", "sat", ["sat_se.fq"], ["-c", "30000"], min_records=SAT_MIN_RECORDS),
]

MIN_RECORDS, MIN_GHOST_READS, MIN_SECONDARY, MIN_LONG_MAPPED = 500, 1000, 50, 2

# the region list of rep_targets: a few hundred kbp inside, the rest outside; one region ends where the next begins
TARGETS = [("chr1", 20_000, 150_000), ("chr1", 250_000, 330_000), ("chr1", 330_000, 340_000), ("chr2", 5_000, 180_000)]

# length lists of test_long_reads and test_reads_beyond_16383_bases (tests/test_gpu_edges_and_properties.py), and a handful
# of the (end 1, end 2, fragment) shapes of test_pairs_with_a_long_end
LONG_LENGTHS = [300, 513, 800, 1024, 1024, 700, 100, 1500, 1025, 64, 2000, 2048, 3000, 5000, 10000, 10000, 1100, 99, 16383, 2500]
LONGER_LENGTHS = [20000, 32766, 17000, 150]
LONG_PAIR_SHAPES = [(1500, 150, 1700), (150, 1500, 1650), (1025, 1025, 1300), (5000, 5000, 6000), (2000, 3000, 4000),
                    (20000, 300, 20400), (17000, 17000, 18000), (10000, 64, 10100)]
TOO_LONG = 32767


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def md5_file(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def write_fastq(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            r = r.decode() if isinstance(r, bytes) else r
            f.write(f"@r{i} edge\n{r}\n+\n{'I' * len(r)}\n")


def _ragged(reads, rng, lo, hi):
    """40 % of the reads cut to lo..hi-1 bases (the lengths whose last seeds see the previous read's buffers), 20 % to a
    length between hi and their own, the rest whole (a few of those are shorter than any read that maps)."""
    out = []
    for r in reads:
        u = rng.random()
        if u < 0.4 and len(r) >= hi:
            r = r[: int(rng.integers(lo, hi))]
        elif u < 0.6 and len(r) >= 60:
            r = r[: int(rng.integers(hi, len(r) + 1))]
        out.append(r)
    return out


def _from_chroms(chroms, lengths, seed, mut=0.02, indel_every=0):
    """Reads of the given lengths cut from the chromosomes, alternating between the first two, every third from the other
    strand, C->T converted, with substitutions and -- for the long ones -- a small indel every few thousand bases (the
    reference's band is 61 wide: a long read may drift by 30 at most)."""
    acgt = synth.ACGT
    rng = np.random.default_rng(seed)
    reads = []
    for k, L in enumerate(lengths):
        ch = chroms[k % 2]
        p = int(rng.integers(1000, len(ch) - L - 1064))
        s = ch[p:p + L + 64].copy()
        if indel_every:
            pieces, at = [], 0
            while at < len(s):
                step = int(rng.integers(indel_every // 2, indel_every * 2))
                pieces.append(s[at:at + step])
                at += step
                if rng.random() < 0.5:
                    at += int(rng.integers(1, 3))
                else:
                    pieces.append(acgt[rng.integers(0, 4, int(rng.integers(1, 3)))])
            s = np.concatenate(pieces)
        s = s[:L].copy()
        if k % 3 == 2:
            s = synth.COMP[s[::-1]]
        s[s == ord("C")] = ord("T")
        m = rng.random(len(s)) < mut
        s[m] = acgt[rng.integers(0, 4, int(m.sum()))]
        reads.append(bytes(s).decode().replace("N", "A"))
    return reads


def _pairs_from_chroms(chroms, shapes, seed):
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    frags = _from_chroms(chroms, [f for _, _, f in shapes], seed=seed, indel_every=2500)
    r1 = [fr[:a] for fr, (a, _, _) in zip(frags, shapes)]
    r2 = [fr[len(fr) - b:].encode().translate(comp)[::-1].decode() for fr, (_, b, _) in zip(frags, shapes)]
    return r1, r2


def _se_at_n_runs(chroms):
    """the single-end reads of test_windows_that_reach_into_an_n_run: cut at distance 0..24 from the long N run, either side
    of it, and from the chromosome's first bases, both strands"""
    reads = []
    for ch in chroms:
        mid = len(ch) // 2
        for L in (100, 97, 150, 300):
            for k in range(25):
                for seg in (ch[mid - L - k: mid - k], ch[mid + 3000 + k: mid + 3000 + k + L],
                            ch[50 + k: 50 + k + L] if ch[0] == ord("N") else ch[k: k + L]):
                    s = seg.copy()
                    s[s == ord("C")] = ord("T")
                    reads.append(bytes(s).decode())
                    reads.append(bytes(synth.COMP[seg[::-1]]).decode().replace("C", "T"))
    return reads


def _across_targets(chroms):
    """reads of 100 bases and pairs (fragments of 260) that step across every boundary of the target regions"""
    names = {"chr1": 0, "chr2": 1}
    se, p1, p2 = [], [], []
    for c, a, b in TARGETS:
        ch = chroms[names[c]]
        for edge in (a, b):
            for k in range(-95, 10, 5):
                s = ch[edge + k: edge + k + 100]
                se.append(bytes(s).decode().replace("C", "T"))
                f = ch[edge + k - 80: edge + k + 180]
                p1.append(bytes(f[:100]).decode().replace("C", "T"))
                p2.append(bytes(synth.COMP[f[::-1]][:100]).decode().replace("G", "A"))
    return se, p1, p2


def make_inputs(wd):
    """Writes every input of the matrix into wd (a few seconds) and returns {file name: md5}."""
    os.makedirs(wd, exist_ok=True)
    p = lambda name: os.path.join(wd, name)
    if not os.path.exists(p("tRex1.fa")):
        os.symlink(os.path.join(GOLD, "tRex1.fa"), p("tRex1.fa"))
    synth.repeat_rich_genome(p("rep.fa"), seed=12, n_chroms=2, chrom_len=400_000, iupac=3000)
    synth.repeat_rich_genome(p("plain.fa"), seed=11, n_chroms=2, chrom_len=400_000)
    with open(p("targets.bed"), "w") as f:
        f.write("".join(f"{c}\t{a}\t{b}\n" for c, a, b in TARGETS))
    rep, plain, trex = (synth.read_chroms(p(x)) for x in ("rep.fa", "plain.fa", "tRex1.fa"))

    # single-end on rep: one draw of reads, cut three ways
    base = synth.mutated_reads(p("rep.fa"), 6000, 120, seed=3, mut=0.03, pbat_frac=0.5)
    se = _ragged(base, np.random.default_rng(7), 44, 47)
    write_fastq(p("se.fq"), se)
    write_fastq(p("se_w12.fq"), _ragged(base, np.random.default_rng(8), 36, 47))
    across_se, across_1, across_2 = _across_targets(rep)
    write_fastq(p("se_targets.fq"), across_se + se)

    # paired-end on rep
    a, b = synth.mutated_pairs(p("rep.fa"), 4000, 110, seed=5, mut=0.03)
    r1, r2 = synth.cut_pairs_ragged(a, b, np.random.default_rng(9), 40, 110)
    write_fastq(p("pe_1.fq"), r1); write_fastq(p("pe_2.fq"), r2)
    write_fastq(p("pbat_1.fq"), r2); write_fastq(p("pbat_2.fq"), r1)
    write_fastq(p("mix_1.fq"), [y if i % 2 else x for i, (x, y) in enumerate(zip(r1, r2))])
    write_fastq(p("mix_2.fq"), [x if i % 2 else y for i, (x, y) in enumerate(zip(r1, r2))])
    s1, s2 = synth.cut_pairs_ragged(a, b, np.random.default_rng(10), 36, 110)
    write_fastq(p("pe_w12_1.fq"), s1); write_fastq(p("pe_w12_2.fq"), s2)
    write_fastq(p("pe_targets_1.fq"), across_1 + r1); write_fastq(p("pe_targets_2.fq"), across_2 + r2)

    # N-run edges on the genome without IUPAC letters
    write_fastq(p("nrun.fq"), _se_at_n_runs(plain))
    n1, n2 = synth.pairs_at_n_runs(plain, (100, 150), seed=4, mirrored=True, straddle=True, unmated=True)
    write_fastq(p("nrun_1.fq"), n1); write_fastq(p("nrun_2.fq"), n2)

    # long reads on tRex1, among ordinary ones
    pad = synth.mutated_reads(p("tRex1.fa"), 700, 100, seed=13, mut=0.02)
    long_ = _from_chroms(trex, LONG_LENGTHS, seed=9, indel_every=3000)
    longer = _from_chroms(trex, LONGER_LENGTHS, seed=10, mut=0.01)
    write_fastq(p("long.fq"), pad[:350] + long_ + pad[350:])
    write_fastq(p("longer.fq"), pad[:200] + longer + pad[200:])
    l1, l2 = _pairs_from_chroms(trex, LONG_PAIR_SHAPES, seed=31)
    q1, q2 = synth.mutated_pairs(p("tRex1.fa"), 400, 100, seed=14)
    write_fastq(p("long_1.fq"), q1[:150] + l1 + q1[150:]); write_fastq(p("long_2.fq"), q2[:150] + l2 + q2[150:])
    write_fastq(p("too_long.fq"), pad[:20] + _from_chroms(trex, [TOO_LONG], seed=11) + pad[20:40])

    # the satellite family (tests/test_gpu_pe_full_sets.py's genomes and reads)
    near = synth.satellite_genome(p("sat.fa"), divergence=0.025, **SAT_FAMILY)
    exact = synth.satellite_genome(p("sat_exact.fa"), divergence=0.0, **SAT_FAMILY)
    t1, t2 = synth.pairs_on_satellite(near, p("sat.fa"), SAT_PAIRS, 100, seed=7, max_frag=40000)
    write_fastq(p("sat_1.fq"), t1); write_fastq(p("sat_2.fq"), t2)
    write_fastq(p("sat_mix_1.fq"), [y if i % 2 else x for i, (x, y) in enumerate(zip(t1, t2))])
    write_fastq(p("sat_mix_2.fq"), [x if i % 2 else y for i, (x, y) in enumerate(zip(t1, t2))])
    e1, e2 = synth.pairs_on_satellite(exact, p("sat_exact.fa"), SAT_PAIRS, 100, seed=7, max_frag=40000, planted=0.0)
    write_fastq(p("sat_exact_1.fq"), e1); write_fastq(p("sat_exact_2.fq"), e2)
    write_fastq(p("sat_se.fq"), synth.reads_on_satellite(near, p("sat.fa"), SAT_READS, 100, seed=11))

    names = sorted({f for c in CASES for f in c["reads"]} | {g for g, _, _ in INDEXES.values()} | {"targets.bed"})
    return {n: md5_file(p(n)) for n in names}


def case_inputs(case):
    """the files a case depends on: its genome, its targets file, its reads"""
    genome, _, targets = INDEXES[case["index"]]
    return [genome] + ([targets] if targets else []) + case["reads"]


# ---- running a case -------------------------------------------------------------------------------------------------------
def idx_command(tool, index, wd, out):
    """`idx` of one of the three command lines ('ref', 'oracle', 'product') for an index of INDEXES"""
    genome, window, targets = INDEXES[index]
    if tool == "ref":
        cmd = [REF_SHORT if window == 12 else REF, "idx"]
    elif tool == "oracle":
        cmd = [ORACLE_CLI, "idx"] + (["-w", "12"] if window == 12 else [])
    else:
        cmd = [PRODUCT_CLI, "idx"] + (["-short"] if window == 12 else [])
    return cmd + (["-A", os.path.join(wd, targets)] if targets else []) + [os.path.join(wd, genome), out]


def build_index(tool, index, wd, out, timeout=600):
    r = subprocess.run(idx_command(tool, index, wd, out), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0 and os.path.exists(out), f"{tool} idx failed for {index}:\n{r.stdout}"
    return out


def map_command(tool, case, wd, idx, out_prefix, extra=()):
    exe = {"ref": REF_SHORT if INDEXES[case["index"]][1] == 12 else REF, "oracle": ORACLE_CLI, "product": PRODUCT_CLI}[tool]
    return ([exe, "map"] + case["flags"] + list(extra) + ["-s", out_prefix + ".stats", "-o", out_prefix + ".sam", "-i", idx] +
            [os.path.join(wd, f) for f in case["reads"]])


def run_map(tool, case, wd, idx, out_prefix, extra=(), env=None, timeout=600):
    """One `map` run; returns the finished process (stdout and stderr together as text)."""
    for ext in (".sam", ".stats"):
        if os.path.exists(out_prefix + ext):
            os.remove(out_prefix + ext)
    return subprocess.run(map_command(tool, case, wd, idx, out_prefix, extra), env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=timeout)


def sam_body(path):
    """the SAM's lines without @PG, the one line that carries the command line"""
    return [ln for ln in open(path, "rb") if not ln.startswith(b"@PG")]


def digest(out_prefix):
    body = sam_body(out_prefix + ".sam")
    return {"records": sum(1 for ln in body if not ln.startswith(b"@")),
            "sam_md5": hashlib.md5(b"".join(body)).hexdigest(),
            "stats_md5": md5_file(out_prefix + ".stats")}


def first_differences(prefix_a, prefix_b, label_a, label_b, n=3):
    """the first n SAM lines at which two runs differ, side by side, and the two statistics files if they differ"""
    a, b = sam_body(prefix_a + ".sam"), sam_body(prefix_b + ".sam")
    out = [f"{label_a}: {len(a)} lines, {label_b}: {len(b)} lines"]
    for i in range(max(len(a), len(b))):
        x = a[i].decode(errors="replace").rstrip("\n") if i < len(a) else "<no line>"
        y = b[i].decode(errors="replace").rstrip("\n") if i < len(b) else "<no line>"
        if x != y:
            out.append(f"line {i + 1}:\n  {label_a}: {x[:400]}\n  {label_b}: {y[:400]}")
            if len(out) > n:
                break
    sa, sb = open(prefix_a + ".stats").read(), open(prefix_b + ".stats").read()
    if sa != sb:
        out.append(f"statistics, {label_a}:\n{sa}\nstatistics, {label_b}:\n{sb}")
    return "\n".join(out)


def refusal(output):
    """the reference's complaint about a read beyond its limit, out of whatever else a failing run printed"""
    lines = [ln[ln.index("found a read"):].strip() for ln in output.splitlines() if "found a read" in ln]
    return lines[0] if lines else ""


def load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def stale_inputs(case_entry, made):
    """names of the case's inputs whose regenerated md5 is not the manifest's"""
    return [n for n, h in case_entry["inputs"].items() if made.get(n) != h]


# ---- the recorder ---------------------------------------------------------------------------------------------------------
def _mapped_fields(out_prefix):
    return [ln.split(b"\t") for ln in sam_body(out_prefix + ".sam") if not ln.startswith(b"@")]


def record(wd):
    for exe in (REF, REF_SHORT):
        if not os.path.exists(exe):
            raise SystemExit(f"{exe} is not built (make -C oracle, with the reference tree present)")
    made = make_inputs(wd)
    ghosts = sum(1 for r in synth.trim_like_readloader([ln.rstrip("\n") for i, ln in enumerate(open(os.path.join(wd, "se.fq"))) if i % 4 == 1])
                 if 44 <= len(r) <= 46)
    assert ghosts >= MIN_GHOST_READS, f"only {ghosts} reads of 44-46 bases in se.fq"
    manifest = {"indexes": {}, "cases": []}
    idx = {}
    for name in INDEXES:
        idx[name] = build_index("ref", name, wd, os.path.join(wd, f"ref_{name}.idx"))
        manifest["indexes"][name] = md5_file(idx[name])
    for case in CASES:
        prefix = os.path.join(wd, "ref_" + case["name"])
        r = run_map("ref", case, wd, idx[case["index"]], prefix)
        entry = {"name": case["name"], "index": case["index"], "flags": case["flags"], "reads": case["reads"],
                 "inputs": {n: made[n] for n in case_inputs(case)}}
        if case.get("refused"):
            assert r.returncode != 0 and "too long" in r.stdout, f"{case['name']}: the reference took the read:\n{r.stdout}"
            entry.update(exit_status=r.returncode, message=refusal(r.stdout))
        else:
            assert r.returncode == 0, f"{case['name']}: the reference failed:\n{r.stdout}"
            entry.update(digest(prefix))
            fields = _mapped_fields(prefix)
            assert entry["records"] >= case.get("min_records", MIN_RECORDS), f"{case['name']}: only {entry['records']} records"
            if "-a" in case["flags"]:
                sec = sum(1 for f in fields if int(f[1]) & 0x100)
                assert sec >= case.get("min_secondary", MIN_SECONDARY), f"{case['name']}: only {sec} records with flag 0x100"
            if case.get("long_reads"):
                n_long = sum(1 for f in fields if len(f[9]) >= 5000)
                assert n_long >= MIN_LONG_MAPPED, f"{case['name']}: only {n_long} mapped reads of 5000 bases or more"
        manifest["cases"].append(entry)
        print(f"{case['name']}: {entry.get('records', entry.get('message'))}", flush=True)
    with open(MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {MANIFEST}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python -m tests.reference_edges --record")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        record(tmp)
