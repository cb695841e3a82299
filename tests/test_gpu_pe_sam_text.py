"""Paired-end SAM text written by the pair kernels (abm_ctx_set_sam_tails + abm_ctx_pe_sam_tails): every pair's records
after QNAME equal the plain-Python formatter of tests/sam_format.py byte for byte, mapping results are the same as
without text, every launch form writes text, and the CLI's output is byte-identical with the text from the device."""
import json
import os
import random
import subprocess

import pytest

from tests import sam_format
from tests.test_gpu_cli_goldens import CLI, chain, golden, md5  # noqa: F401 (chain: the goldens' fixture)
from tests.test_gpu_pe_parity import sim_pairs

pytestmark = pytest.mark.gpu


def same_results(a, b, label):
    pa, s1a, s2a, (c1a, o1a), (c2a, o2a) = a[:5]
    pb, s1b, s2b, (c1b, o1b), (c2b, o2b) = b[:5]
    assert pa.tobytes() == pb.tobytes(), f"{label}: pairs differ with SAM text on"
    assert s1a.tobytes() == s1b.tobytes() and s2a.tobytes() == s2b.tobytes(), f"{label}: fallback hits differ"
    assert (c1a == c1b).all() and (o1a == o1b).all() and (c2a == c2b).all() and (o2a == o2b).all(), f"{label}: CIGARs differ"


def check_text(ix, r1, r2, res, allow_ambig, label, min_device=0.95):
    """the device's tails against tests/sam_format.py; returns the kinds"""
    kinds, tails = res[5], res[6]
    assert kinds is not None, f"{label}: the batch wrote no SAM text"
    want = sam_format.format_batch(allow_ambig, ix, r1, r2, res)
    bad = []
    for i, (k, (t1, t2)) in enumerate(zip(kinds, tails)):
        if int(k) == 0xFF:
            assert t1 == b"" and t2 == b"", f"{label}: pair {i} left to the host has text"
            continue
        if (int(k), t1, t2) != want[i]:
            bad.append((i, (int(k), t1, t2), want[i]))
    assert not bad, f"{label}: {len(bad)} of {len(kinds)} pairs differ; first: {bad[:2]}"
    done = sum(1 for k in kinds if int(k) != 0xFF)
    assert done >= min_device * len(kinds), f"{label}: only {done} of {len(kinds)} pairs formatted on the device"
    return kinds


def mapped_twice(ctx, r1, r2, mode, allow_ambig, params=None):
    import abismal_amd as A
    params = params or A.Params(allow_ambig=1 if allow_ambig else 0)
    ctx.set_sam_tails(False)
    plain = ctx.map_pe(r1, r2, mode=mode, params=params)
    ctx.set_sam_tails(True, allow_ambig=allow_ambig)
    try:
        text = ctx.map_pe(r1, r2, mode=mode, params=params, sam=True)
    finally:
        ctx.set_sam_tails(False)
    return plain, text


@pytest.fixture(scope="module")
def trex(trex_index):
    import abismal_amd as A
    ix = A.Index(trex_index)
    ctx = A.Context(ix, 0)
    yield ix, ctx
    ctx.close()
    ix.close()


@pytest.mark.parametrize("allow_ambig", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_trex_pairs_text_equals_formatter(oracle, workdir, trex, mode, allow_ambig):
    ix, ctx = trex
    kw = {1: dict(pbat=True), 2: dict(random_pbat=True)}.get(mode, {})
    r1, r2 = sim_pairs(oracle, workdir, f"samtext_{mode}", n=4000, **kw)
    plain, text = mapped_twice(ctx, r1, r2, mode, allow_ambig)
    same_results(plain, text, f"mode {mode}")
    kinds = check_text(ix, r1, r2, text, allow_ambig, f"tRex1 mode {mode} allow_ambig {allow_ambig}")
    assert sum(1 for k in kinds if int(k) == 0) > 0.5 * len(kinds)
    assert ctx.pinned_bytes() >= len(r1) * 2 * 200, "pinned_bytes counts the SAM slots"


def test_every_launch_form_writes_text(trex_index, workdir):
    import abismal_amd as A
    from tests import synth
    from tests.test_gpu_pe_split import FORMS
    fa = os.path.join(workdir, "rep_pe_samtext.fa")
    idx = os.path.join(workdir, "rep_pe_samtext.idx")
    synth.repeat_rich_genome(fa)
    A.index_build(fa, idx, 8)
    r1, r2 = synth.mutated_pairs(fa, 3000, 100, seed=211)
    r1, r2 = synth.trim_like_readloader(r1), synth.trim_like_readloader(r2)
    ix = A.Index(idx)
    ctx = A.Context(ix, 0)
    routes = {"mated_from_lds": 0, "mapped_whole": 0, "mated_from_device_memory": 0}
    try:
        for form, kw in FORMS:
            ctx.set_pe_split(**kw)
            plain = ctx.map_pe(r1, r2, mode=0)
            ctx.pe_split_stats()
            ctx.set_sam_tails(True)
            text = ctx.map_pe(r1, r2, mode=0, sam=True)
            ctx.set_sam_tails(False)
            st = ctx.pe_split_stats()
            same_results(plain, text, form)
            check_text(ix, r1, r2, text, False, f"repeat-rich, {form}", min_device=0.9)
            for k in routes:
                routes[k] += st[k]
    finally:
        ctx.close()
        ix.close()
    assert all(v > 0 for v in routes.values()), routes


def _pick(fa_seq, rng, L):
    p = rng.randrange(0, len(fa_seq) - 2000)
    return p, fa_seq[p:p + L]


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgtN", "TGCAtgcaN"))


def _bisulfite(s):
    return s.replace("C", "T")


def test_odd_pairs(trex, trex_index):
    """IUPAC letters, ends of 44-46 bases, an end below min_len, ends on two chromosomes; long ends (>1024 bases) leave
    their batch to the host"""
    ix, ctx = trex
    names = ix.chrom_names
    fa = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tRex1.fa")
    chroms, cur = {}, None
    for line in open(fa):
        line = line.strip()
        if line.startswith(">"):
            cur = line[1:].split()[0]
            chroms[cur] = []
        elif cur:
            chroms[cur].append(line.upper())
    seqs = {k: "".join(v) for k, v in chroms.items()}
    keys = list(seqs)
    rng = random.Random(7)
    r1, r2, what = [], [], []

    def add(a, b, tag):
        r1.append(a)
        r2.append(b)
        what.append(tag)

    for _ in range(40):  # IUPAC letters in the reads
        p, frag = _pick(seqs[keys[0]], rng, 300)
        a, b = list(_bisulfite(frag[:100])), list(_bisulfite(_revcomp(frag[-100:])))
        for s in (a, b):
            for _k in range(3):
                s[rng.randrange(len(s))] = rng.choice("RYKMSWBDHVn")
        add("".join(a), "".join(b), "iupac")
    for L in (44, 45, 46):  # ends where seeds reach past the end of the read
        for _ in range(10):
            p, frag = _pick(seqs[keys[0]], rng, 250)
            add(_bisulfite(frag[:L]), _bisulfite(_revcomp(frag[-L:])), f"len{L}")
    for _ in range(10):  # one end below min_len
        p, frag = _pick(seqs[keys[0]], rng, 250)
        add(_bisulfite(frag[:100]), _bisulfite(_revcomp(frag[-20:])), "short")
    for _ in range(10):  # unrelated ends on two chromosomes: never mated, the single-end fallback (the mated case:
        # test_pair_mated_across_a_chromosome_join)
        _, f1 = _pick(seqs[keys[0]], rng, 150)
        _, f2 = _pick(seqs[keys[1 % len(keys)]], rng, 150)
        add(_bisulfite(f1[:120]), _bisulfite(_revcomp(f2[-120:])), "two_chroms")
    import abismal_amd as A
    params = A.Params(max_frag=3000)
    # long ends (beyond 1024 bases: the long-end launch's) in a batch with ordinary pairs: such a batch is filtered on the
    # nibble array (ends beyond 448 bases), whose builds write no text -- the whole batch is the host's, results unchanged
    l1, l2 = list(r1[:20]), list(r2[:20])
    for L1, L2 in ((1500, 150), (150, 1100)):
        p, frag = _pick(seqs[keys[0]], rng, 1800)
        l1.append(_bisulfite(frag[:L1]))
        l2.append(_bisulfite(_revcomp(frag[-L2:])))
    plain, text = mapped_twice(ctx, l1, l2, 0, False, params=params)
    same_results(plain, text, "pairs with long ends")
    assert text[5] is None and text[6] is None
    plain, text = mapped_twice(ctx, r1, r2, 0, False, params=params)
    same_results(plain, text, "odd pairs")
    kinds = check_text(ix, r1, r2, text, False, "odd pairs", min_device=0.0)
    for k, tag in zip(kinds, what):
        if tag == "two_chroms":
            assert int(k) == 1, "unrelated ends: single-end records"
        else:
            assert int(k) != 0xFF, tag
    assert any(int(k) == 0 for k, t in zip(kinds, what) if t == "iupac")
    assert names  # (the formatter read the index's chromosome table)


def _run(chain, args, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([CLI, "map"] + args, cwd=chain, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


PE_GOLDENS = [
    (["-s", "tests/reads_pe.mstats", "-o", "tests/reads_pe.sam", "-i", "tests/tRex1.idx", "tests/reads_pe_1.fq",
      "tests/reads_pe_2.fq"], ["tests/reads_pe.sam", "tests/reads_pe.mstats"]),
    (["-P", "-s", "tests/reads_pbat_pe.mstats", "-o", "tests/reads_pbat_pe.sam", "-i", "tests/tRex1.idx",
      "tests/reads_pbat_pe_1.fq", "tests/reads_pbat_pe_2.fq"], ["tests/reads_pbat_pe.sam", "tests/reads_pbat_pe.mstats"]),
    (["-P", "-s", "tests/reads_rpbat_pe.mstats", "-o", "tests/reads_rpbat_pe.sam", "-i", "tests/tRex1.idx",
      "tests/reads_rpbat_pe_1.fq", "tests/reads_rpbat_pe_2.fq"], ["tests/reads_rpbat_pe.sam", "tests/reads_rpbat_pe.mstats"]),
]


@pytest.mark.parametrize("args,outs", PE_GOLDENS)
def test_cli_pe_goldens_with_device_text(chain, args, outs):
    _run(chain, args, {"ABM_CLI_DEVICE_SAM": "1"})
    g = golden()
    for rel in outs:
        if rel in g:
            assert md5(chain / rel) == g[rel], rel


@pytest.mark.parametrize("extra", [[], ["-a"], ["-R"]])
@pytest.mark.parametrize("small", [False, True])
def test_cli_pe_device_text_is_byte_identical(chain, extra, small):
    base = ["-i", "tests/tRex1.idx", "tests/reads_pe_1.fq", "tests/reads_pe_2.fq"]
    env = {"ABM_CLI_BATCH_READS": "3000", "ABM_CLI_SLICE_READS": "997"} if small else {}
    outs = {}
    for dev in ("0", "1"):
        sam, st, tj = f"tests/dt{dev}.sam", f"tests/dt{dev}.mstats", f"tests/dt{dev}.json"
        _run(chain, extra + ["-timing", tj, "-s", st, "-o", sam] + base, dict(env, ABM_CLI_DEVICE_SAM=dev))
        body = [l for l in open(chain / sam, "rb") if not l.startswith(b"@PG")]
        outs[dev] = (body, open(chain / st, "rb").read(), json.load(open(chain / tj)))
    assert outs["0"][0] == outs["1"][0] and len(outs["1"][0]) > 15000
    assert outs["0"][1] == outs["1"][1]
    t0, t1 = outs["0"][2], outs["1"][2]
    assert t0["sam_text_by"] == "host" and t0["sam_records"]["device"] == 0
    assert t1["sam_text_by"] == "device" and t1["sam_records"]["device"] > 0.9 * len(outs["1"][0])
    assert t1["sam_records"]["device"] + t1["sam_records"]["host"] == t0["sam_records"]["host"]


# ---- pairs the device hands back, and pairs mated across a chromosome join -------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fasta(path):
    seqs, cur = {}, None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            cur = line[1:].split()[0]
            seqs[cur] = []
        elif cur:
            seqs[cur].append(line.upper())
    return {k: "".join(v) for k, v in seqs.items()}


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def _conv(s):
    return s.replace("C", "T")


def many_op_pairs(seqs, n, seed=5, blocks=13, L1=400, L2=150):
    """pairs whose read 1 aligns with a CIGAR of about 53 ops -- more than the 50 the kernels keep in LDS (CigarSink::fin):
    13 blocks of an inserted base, four reference bases and a deleted one (26 edits of 40 allowed), placed where the four
    bases shifted by one would all mismatch, so that the alignment takes the two indels"""
    rng = random.Random(seed)
    g = max(seqs.values(), key=len)
    out1, out2 = [], []
    while len(out1) < n:
        p = rng.randrange(1000, len(g) - 3000)
        fc = _conv(g[p:p + 900])
        if "N" in fc:
            continue
        parts, i, b = [fc[:120]], 120, 0
        while b < blocks:
            w = fc[i:i + 5]
            if all(w[j] != w[j + 1] for j in range(4)):
                parts.append(rng.choice([c for c in "AGT" if c != w[0]]) + fc[i:i + 4])  # then fc[i + 4] is deleted
                parts.append(fc[i + 5:i + 13])
                i += 13
                b += 1
            else:
                parts.append(fc[i])
                i += 1
        r1 = "".join(parts)
        need = L1 - len(r1)
        if need < 20:  # (ends stay within 448 bases: the launches with SAM text filter on the bit planes)
            continue
        r1 += fc[i:i + need]
        e = i + need + 120
        out1.append(r1)
        out2.append(_rc(fc[e - L2:e]))
    return out1, out2


def join_pairs(seqs, names, starts, L=120):
    """pairs whose fragment spans the join of two chromosomes adjacent in the index: read 1 from the last bases of one,
    read 2 (reverse-complemented) from just past the N run the next one opens with (tRex1's chr2: 10,000 Ns, so the
    fragments are ~12 kb).  The mapper mates them; SAM cannot: unmapped as a pair"""
    out1, out2 = [], []
    for k in range(len(names) - 1):
        a, b = names[k], names[k + 1]
        if a not in seqs or b not in seqs or int(starts[k + 1]) - int(starts[k]) != len(seqs[a]):
            continue
        lead = len(seqs[b]) - len(seqs[b].lstrip("N"))
        for j in range(6):
            back = 130 + 37 * j
            s1 = seqs[a][len(seqs[a]) - back:len(seqs[a]) - back + L]
            s2 = seqs[b][lead + 1800 + 23 * j:lead + 1800 + 23 * j + L]  # (nearer the N run read 2 is ambiguous)
            if "N" not in s1 and "N" not in s2:
                out1.append(_conv(s1))
                out2.append(_rc(_conv(s2)))
    return out1, out2


def test_cigars_beyond_fin_are_left_to_the_host(oracle, workdir, trex):
    """a pair whose CIGAR has more ops than fin holds comes out as kind 0xFF with no text, in the middle of a batch whose
    other pairs' text stays right"""
    ix, ctx = trex
    seqs = _fasta(os.path.join(GOLD, "tRex1.fa"))
    m1, m2 = many_op_pairs(seqs, 20)
    s1, s2 = sim_pairs(oracle, workdir, "samtext_fin", n=600)
    r1 = s1[:300] + [x for pair in zip(m1, s1[300:320]) for x in pair] + s1[320:]
    r2 = s2[:300] + [x for pair in zip(m2, s2[300:320]) for x in pair] + s2[320:]
    many = set(range(300, 340, 2))
    plain, text = mapped_twice(ctx, r1, r2, 0, False)
    same_results(plain, text, "CIGARs beyond fin")
    kinds = check_text(ix, r1, r2, text, False, "CIGARs beyond fin", min_device=0.9)
    c1, o1 = text[3]
    tails = text[6]
    beyond = [i for i in many if int(o1[i + 1] - o1[i]) > 50]
    assert len(beyond) >= 15, "the fixture's read 1 must align with more than 50 ops"
    for i in beyond:
        assert int(text[0][i]["r1"]["pos"]) != 0, "the fixture's pairs must map"
        assert int(kinds[i]) == 0xFF and tails[i] == (b"", b""), (i, int(kinds[i]))
    for i in range(len(r1)):  # the neighbours of those pairs, and the rest of the batch
        if i not in many:
            assert int(kinds[i]) != 0xFF, i


def test_pair_mated_across_a_chromosome_join(trex):
    """a pair the mapper reports whose ends lie on two chromosomes: kind 1 (unmapped as a pair), no records -- its
    fallback hits were never computed"""
    import abismal_amd as A
    ix, ctx = trex
    seqs = _fasta(os.path.join(GOLD, "tRex1.fa"))
    j1, j2 = join_pairs(seqs, ix.chrom_names, ix.chrom_starts)
    assert len(j1) >= 4
    plain, text = mapped_twice(ctx, j1, j2, 0, False, params=A.Params(max_frag=15000))
    same_results(plain, text, "pairs across a chromosome join")
    kinds = check_text(ix, j1, j2, text, False, "pairs across a chromosome join", min_device=1.0)
    starts = ix.chrom_starts
    for i in range(len(j1)):
        p = text[0][i]
        assert int(p["r1"]["pos"]) != 0, "the mapper reports the pair"
        assert int(p["r1"]["pos"]) < int(starts[2]) <= int(p["r2"]["pos"]), "its ends lie on chr1 and chr2"
        assert int(kinds[i]) == 1 and text[6][i] == (b"", b""), (i, int(kinds[i]), text[6][i])


def test_cli_odd_pairs_byte_identical(chain):
    """CIGARs beyond fin and pairs mated across the chromosome join amid ordinary pairs, through the CLI: the same SAM and
    statistics with the device's text as with the host's, and both wrote records in the one run"""
    import abismal_amd as A
    seqs = _fasta(os.path.join(GOLD, "tRex1.fa"))
    ix = A.Index(str(chain / "tests/tRex1.idx"))
    try:
        j1, j2 = join_pairs(seqs, ix.chrom_names, ix.chrom_starts)
    finally:
        ix.close()
    m1, m2 = many_op_pairs(seqs, 30, seed=9)
    odd = list(zip(m1, m2)) + list(zip(j1, j2))
    for e, src in ((0, "tests/reads_pe_1.fq"), (1, "tests/reads_pe_2.fq")):
        lines = open(chain / src).read().splitlines()
        recs = [lines[k:k + 4] for k in range(0, 4 * 3000, 4)]
        out = []
        for k, rec in enumerate(recs):
            out += rec
            if k % 90 == 45 and k // 90 < len(odd):
                s = odd[k // 90][e]
                out += [f"@odd{k // 90}", s, "+", "B" * len(s)]
        open(chain / f"tests/odd_{e + 1}.fq", "w").write("\n".join(out) + "\n")
    outs = {}
    for dev in ("0", "1"):
        sam, st, tj = f"tests/odd{dev}.sam", f"tests/odd{dev}.mstats", f"tests/odd{dev}.json"
        _run(chain, ["-L", "15000", "-timing", tj, "-s", st, "-o", sam, "-i", "tests/tRex1.idx", "tests/odd_1.fq",
                     "tests/odd_2.fq"], {"ABM_CLI_DEVICE_SAM": dev, "ABM_CLI_BATCH_READS": "1000", "ABM_CLI_SLICE_READS": "333"})
        body = [l for l in open(chain / sam, "rb") if not l.startswith(b"@PG")]
        outs[dev] = (body, open(chain / st, "rb").read(), json.load(open(chain / tj)))
    assert outs["0"][0] == outs["1"][0] and len(outs["1"][0]) > 5000
    assert outs["0"][1] == outs["1"][1]
    t1 = outs["1"][2]
    assert t1["sam_text_by"] == "device"
    assert t1["sam_records"]["device"] > 0 and t1["sam_records"]["host"] > 0, t1["sam_records"]
    assert t1["sam_records"]["device"] + t1["sam_records"]["host"] == outs["0"][2]["sam_records"]["host"]
    assert any(l.startswith(b"odd0\t") for l in outs["1"][0]), "the pairs with long CIGARs have records"
