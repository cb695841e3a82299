"""BAM pieces written by the mapping kernels (abm_ctx_set_record_format(ABM_RECORDS_BAM) on top of abm_ctx_set_sam_tails):
every piece equals tests/bam_format.py over the returned hits and CIGARs byte for byte, mapping results are what they
are without records, a reserved context regrows nothing, `abismal-amd map -B` writes the same stream with the device's
pieces as with the host's records, and the writer alone takes the fields no small genome reaches."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import bam_format, sam_format
from tests.test_gpu_cli_goldens import CLI, chain  # noqa: F401 (chain: the goldens' fixture)
from tests.test_gpu_pe_parity import sim_pairs
from tests.test_gpu_pe_sam_text import same_results

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SE_SLOT_OPS, PE_FIN_OPS = 4, 50


@pytest.fixture(scope="module")
def trex(trex_index):
    import abismal_amd as A
    ix = A.Index(trex_index)
    ctx = A.Context(ix, 0)
    yield ix, ctx
    ctx.close()
    ix.close()


@pytest.fixture(scope="module")
def genome():
    seqs, cur = {}, None
    for line in open(os.path.join(GOLD, "tRex1.fa")):
        line = line.strip()
        if line.startswith(">"):
            cur = line[1:].split()[0]
            seqs[cur] = []
        elif cur:
            seqs[cur].append(line.upper())
    return max(("".join(v) for v in seqs.values()), key=len)


def alive(o_res, o_n, n_reads, slot_ops, label):
    """the oracle's own output: the batch maps, and few CIGARs are beyond the slot"""
    mapped = int((np.asarray(o_res["pos"]) != 0).sum())
    beyond = int((np.asarray(o_n) > slot_ops).sum())
    print(f"{label}: oracle maps {mapped} of {n_reads}, {beyond} CIGARs beyond {slot_ops} ops")
    assert mapped > 0.8 * n_reads, f"{label}: the oracle maps only {mapped} of {n_reads}"
    assert beyond <= 0.02 * n_reads, f"{label}: {beyond} CIGARs beyond the slot"


def table(ix):
    names = list(ix.chrom_names)
    return names, [int(x) for x in ix.chrom_starts[:len(names) + 1]]


def want_se(allow_ambig, starts, h, seq, cig):
    """emit_se + put_bam_record, without the name"""
    flags, pos = int(h["flags"]), int(h["pos"])
    amb = bool(flags & 0x100)
    if pos == 0 or not seq or (amb and not allow_ambig):
        return b""
    loc = sam_format.locate(starts, pos, sam_format.ref_len(cig))
    if loc is None:
        return b""
    rc = bool(flags & 0x10)
    return bam_format.piece((0x10 if rc else 0) | (0x100 if allow_ambig and amb else 0), loc[0] - 1, loc[1], cig, "*", 0, 0, seq, rc,
                            int(h["diffs"]), "A" if flags & 0x1000 else "T")


def check_se(ix, ctx, reads, first, mode, allow_ambig, label, min_device):
    import abismal_amd as A
    params = A.Params(allow_ambig=1 if allow_ambig else 0)
    ctx.set_sam_tails(False)
    plain = ctx.map_se_sliced(reads, first, mode=mode, params=params)
    ctx.set_sam_tails(True, allow_ambig=allow_ambig)
    ctx.set_record_format(bam=True)
    try:
        res, cig, off, _, recs = ctx.map_se_sliced(reads, first, mode=mode, params=params, tails=True)
    finally:
        ctx.set_sam_tails(False)
        ctx.set_record_format(bam=False)
    assert res.tobytes() == plain[0].tobytes() and (cig == plain[1]).all() and (off == plain[2]).all(), f"{label}: results differ with records on"
    _, starts = table(ix)
    lo = int(first[0])
    assert all(r is None for r in recs[:lo]), "reads of the lead-in have no records"
    bad, device, records = [], 0, 0
    for i in range(lo, len(reads)):
        c = cig[int(off[i]):int(off[i + 1])]
        want = want_se(allow_ambig, starts, res[i], reads[i], c)
        records += want != b""
        if recs[i] is None:
            continue
        device += recs[i] != b""
        if recs[i] != want:
            bad.append((i, len(reads[i]), recs[i], want))
    assert not bad, f"{label}: {len(bad)} pieces differ; first: {bad[:1]}"
    assert device >= min_device * records, f"{label}: only {device} of {records} records came from the device"
    return res, cig, off, recs


@pytest.mark.parametrize("allow_ambig", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_single_end_pieces_equal_the_formatter(oracle, workdir, trex_index, trex, mode, allow_ambig):
    from tests import oracle_binding as ob
    ix, ctx = trex
    prefix = os.path.join(workdir, "bam_se")
    if not os.path.exists(prefix + "_1.fq"):
        oracle.simulate(os.path.join(GOLD, "tRex1.fa"), prefix, 2000, single_end=True, seed=41, mut=0.003)  # (at the default 0.01 a ninth of the reads have two indels: beyond the 4-op slot)
    _, reads = ob.read_fastq_like_readloader(prefix + "_1.fq")
    assert len(reads) == 2000 and max(len(r) for r in reads) == 100
    if mode == 1:  # the A-rich mode's reads: the simulator's T-rich ones from the other strand
        reads = [_rc(r) for r in reads]
    oix = oracle.index_load(trex_index)
    try:
        o_res, _, o_n, _ = oracle.map_se(oix, reads, mode=mode)
    finally:
        oracle.index_free(oix)
    alive(o_res, o_n, len(reads), SE_SLOT_OPS, f"tRex1 mode {mode}")
    # three uneven slices after a lead-in of 37 reads
    check_se(ix, ctx, reads, [37, 300, 1531, len(reads)], mode, allow_ambig, f"tRex1 mode {mode} allow_ambig {allow_ambig}", 0.95)


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def ragged_reads(g, seed=3):
    """every length from 44 to 200 (odd and even; the lane rounds at 64 and 128 bases and packed bytes), 250 and 1024
    bases, both strands, a read too short to map, IUPAC and lower-case letters, reads that need five or more CIGAR ops"""
    rng = random.Random(seed)

    def take(L):
        while True:
            p = rng.randrange(1000, len(g) - 3000)
            s = g[p:p + L]
            if "N" not in s:  # (either strand, then the conversion)
                return (_rc(s) if rng.random() < 0.5 else s).replace("C", "T")

    reads, tags = [], []
    for L in list(range(44, 201)) * 12 + [250] * 8 + [1024] * 8:
        s = take(L)
        reads.append(s)
        tags.append("plain")
    for _ in range(20):
        s = list(take(100))
        for _k in range(3):
            s[rng.randrange(100)] = rng.choice("RYKMSWBDHVn")
        for _k in range(5):
            j = rng.randrange(100)
            s[j] = s[j].lower()
        reads.append("".join(s))
        tags.append("iupac")
    for _ in range(20):  # three small deletions and an insertion: five or more CIGAR ops
        s = take(140)
        j = rng.randrange(5, 60)
        reads.append(s[:j] + s[j + 2:j + 10] + "A" + s[j + 10:j + 18] + s[j + 19:j + 30] + s[j + 32:])
        tags.append("many_ops")
    reads.insert(700, take(30))
    tags.insert(700, "short")
    return reads, tags


def test_lengths_where_the_packing_can_go_wrong(oracle, trex_index, trex, genome):
    ix, ctx = trex
    reads, tags = ragged_reads(genome)
    oix = oracle.index_load(trex_index)
    try:
        o_res, _, o_n, _ = oracle.map_se(oix, reads, mode=0)
    finally:
        oracle.index_free(oix)
    alive(o_res, o_n, len(reads), SE_SLOT_OPS, "ragged batch")
    res, cig, off, recs = check_se(ix, ctx, reads, [0, 900, len(reads)], 0, False, "ragged batch", 0.9)
    lengths = {len(r) for r, rec in zip(reads, recs) if rec}
    assert set(range(47, 201)) <= lengths and 250 in lengths and 1024 in lengths, sorted(set(range(44, 201)) - lengths)
    assert any(rec for rec, r in zip(recs, reads) if len(r) in (44, 45, 46))
    strands = {int(res[i]["flags"]) & 0x10 for i, rec in enumerate(recs) if rec}
    assert strands == {0, 0x10}
    assert recs[tags.index("short")] == b""
    assert sum(1 for rec, t in zip(recs, tags) if t == "iupac" and rec) >= 10
    n_ops = [int(off[i + 1] - off[i]) for i in range(len(reads))]
    many = [i for i, t in enumerate(tags) if t == "many_ops" and n_ops[i] >= 5]
    assert len(many) >= 10, "the fixture's reads must align with five or more ops"
    # (an ambiguous hit that is left out has no record whatever its CIGAR: b"")
    assert all(recs[i] is None or (recs[i] == b"" and int(res[i]["flags"]) & 0x100) for i in many), "a CIGAR beyond its 4-op slot is the host's"
    assert sum(1 for i in many if recs[i] is None) >= 10
    assert all(recs[i] is not None for i in range(len(reads)) if n_ops[i] <= 4)


# ---- pairs ------------------------------------------------------------------------------------------------------------
def check_pairs(ix, r1, r2, res, allow_ambig, label, min_device):
    kinds, pieces = res[5], res[6]
    assert kinds is not None, f"{label}: the batch wrote no records"
    names, _ = table(ix)
    refids = {n: i - 1 for i, n in enumerate(names)}
    want = sam_format.format_batch(allow_ambig, ix, r1, r2, res)
    bad = []
    for i, (k, (p1, p2)) in enumerate(zip(kinds, pieces)):
        if int(k) == 0xFF:
            assert p1 == b"" and p2 == b"", f"{label}: pair {i} left to the host has pieces"
            continue
        w = (want[i][0], bam_format.piece_from_tail(want[i][1], refids), bam_format.piece_from_tail(want[i][2], refids))
        if (int(k), p1, p2) != w:
            bad.append((i, (int(k), p1, p2), w))
    assert not bad, f"{label}: {len(bad)} of {len(kinds)} pairs differ; first: {bad[:1]}"
    done = sum(1 for k in kinds if int(k) != 0xFF)
    assert done >= min_device * len(kinds), f"{label}: only {done} of {len(kinds)} pairs written on the device"
    return kinds


def mapped_twice(ctx, r1, r2, mode, allow_ambig, params=None):
    import abismal_amd as A
    params = params or A.Params(allow_ambig=1 if allow_ambig else 0)
    ctx.set_sam_tails(False)
    plain = ctx.map_pe(r1, r2, mode=mode, params=params)
    ctx.set_sam_tails(True, allow_ambig=allow_ambig)
    ctx.set_record_format(bam=True)
    try:
        text = ctx.map_pe(r1, r2, mode=mode, params=params, sam=True)
    finally:
        ctx.set_sam_tails(False)
        ctx.set_record_format(bam=False)
    return plain, text


@pytest.mark.parametrize("allow_ambig", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pairs_pieces_equal_the_formatter(oracle, workdir, trex_index, trex, mode, allow_ambig):
    ix, ctx = trex
    kw = {1: dict(pbat=True), 2: dict(random_pbat=True)}.get(mode, {})
    r1, r2 = sim_pairs(oracle, workdir, f"bam_{mode}", n=2000, **kw)
    oix = oracle.index_load(trex_index)
    try:
        orc = oracle.map_pe(oix, r1, r2, mode=mode)
    finally:
        oracle.index_free(oix)
    alive(orc[0]["r1"], np.maximum(orc[3][1], orc[4][1]), len(r1), PE_FIN_OPS, f"tRex1 pairs mode {mode}")
    plain, text = mapped_twice(ctx, r1, r2, mode, allow_ambig)
    same_results(plain, text, f"mode {mode}")
    kinds = check_pairs(ix, r1, r2, text, allow_ambig, f"tRex1 pairs mode {mode} allow_ambig {allow_ambig}", 0.95)
    assert sum(1 for k in kinds if int(k) == 0) > 0.5 * len(kinds)


def test_every_launch_form_writes_pieces(workdir):
    import abismal_amd as A
    from tests import synth
    from tests.test_gpu_pe_split import FORMS
    fa = os.path.join(workdir, "rep_pe_bam.fa")
    idx = os.path.join(workdir, "rep_pe_bam.idx")
    synth.repeat_rich_genome(fa)
    A.index_build(fa, idx, 8)
    r1, r2 = synth.mutated_pairs(fa, 1500, 100, seed=211)
    r1, r2 = synth.trim_like_readloader(r1), synth.trim_like_readloader(r2)
    ix = A.Index(idx)
    ctx = A.Context(ix, 0)
    routes = {"mated_from_lds": 0, "mapped_whole": 0, "mated_from_device_memory": 0}
    try:
        for form, kw in FORMS:
            ctx.set_pe_split(**kw)
            ctx.pe_split_stats()
            plain, text = mapped_twice(ctx, r1, r2, 0, False)
            st = ctx.pe_split_stats()
            same_results(plain, text, form)
            check_pairs(ix, r1, r2, text, False, f"repeat-rich, {form}", 0.9)
            for k in routes:
                routes[k] += st[k]
    finally:
        ctx.close()
        ix.close()
    assert all(v > 0 for v in routes.values()), routes


def test_odd_pairs(trex, genome):
    """ends on two chromosomes give single-end records; a batch with an end beyond 1,024 bases writes nothing"""
    import abismal_amd as A
    ix, ctx = trex
    seqs, cur = {}, None
    for line in open(os.path.join(GOLD, "tRex1.fa")):
        line = line.strip()
        if line.startswith(">"):
            cur = line[1:].split()[0]
            seqs[cur] = []
        elif cur:
            seqs[cur].append(line.upper())
    seqs = {k: "".join(v) for k, v in seqs.items()}
    keys = list(seqs)
    rng = random.Random(7)

    def pick(s, L):
        p = rng.randrange(0, len(s) - 2000)
        return s[p:p + L]

    r1, r2, what = [], [], []
    for _ in range(40):
        frag = pick(seqs[keys[0]], 300)
        r1.append(frag[:101].replace("C", "T"))
        r2.append(_rc(frag[-99:]).replace("C", "T"))
        what.append("plain")
    for _ in range(10):
        f1, f2 = pick(seqs[keys[0]], 150), pick(seqs[keys[1 % len(keys)]], 150)
        r1.append(f1[:120].replace("C", "T"))
        r2.append(_rc(f2[-120:]).replace("C", "T"))
        what.append("two_chroms")
    params = A.Params(max_frag=3000)
    plain, text = mapped_twice(ctx, r1, r2, 0, False, params=params)
    same_results(plain, text, "odd pairs")
    kinds = check_pairs(ix, r1, r2, text, False, "odd pairs", 0.0)
    assert all(int(k) == 1 for k, t in zip(kinds, what) if t == "two_chroms")
    assert any(int(k) == 0 for k, t in zip(kinds, what) if t == "plain")
    frag = pick(seqs[keys[0]], 1800)
    l1, l2 = r1[:20] + [frag[:1500].replace("C", "T")], r2[:20] + [_rc(frag[-150:]).replace("C", "T")]
    plain, text = mapped_twice(ctx, l1, l2, 0, False, params=params)
    same_results(plain, text, "pairs with a long end")
    assert text[5] is None and text[6] is None


def test_unknown_format_is_refused_and_the_format_kept(oracle, workdir, trex):
    """a real context: format 7 is an error with a text, and the context goes on writing what it wrote before"""
    import ctypes as C
    import abismal_amd as A
    ix, ctx = trex
    lib = A.load_library()
    lib.abm_ctx_set_record_format.argtypes = [C.c_void_p, C.c_int]
    lib.abm_ctx_set_record_format.restype = C.c_int
    lib.abm_last_error.restype = C.c_char_p
    r1, r2 = sim_pairs(oracle, workdir, "bam_0", n=2000)
    r1, r2 = r1[:200], r2[:200]
    ctx.set_sam_tails(True)
    try:
        for bam in (True, False):
            ctx.set_record_format(bam=bam)
            assert lib.abm_ctx_set_record_format(ctx.handle, 7) < 0
            assert b"format" in lib.abm_last_error()
            assert lib.abm_ctx_set_record_format(ctx.handle, -1) < 0
            res = ctx.map_pe(r1, r2, sam=True)
            if bam:
                check_pairs(ix, r1, r2, res, False, "after a refused format, BAM", 0.9)
            else:
                from tests.test_gpu_pe_sam_text import check_text
                check_text(ix, r1, r2, res, False, "after a refused format, SAM", 0.9)
    finally:
        ctx.set_sam_tails(False)
        ctx.set_record_format(bam=False)


# ---- a reserved context --------------------------------------------------------------------------------------------------
def test_reserved_context_regrows_no_buffer(trex_index, monkeypatch, capfd):
    import abismal_amd as A
    from tests import synth
    n, L = 4096, 100
    a, b = synth.mutated_pairs(os.path.join(GOLD, "tRex1.fa"), n + n // 8, L, seed=29)
    keep = [(x, y) for x, y in zip(a, b) if len(x) == L and len(y) == L][:n]
    assert len(keep) == n
    r1, r2 = [x for x, _ in keep], [y for _, y in keep]
    monkeypatch.setenv("ABM_TRACE_HOST", "1")
    ix = A.Index(trex_index)
    try:
        for paired in (False, True):
            capfd.readouterr()
            ctx = A.Context(ix, 0)
            try:
                ctx.set_sam_tails(True)
                ctx.set_record_format(bam=True)
                ctx.reserve(n, L, paired=paired)
                if paired:
                    out = ctx.map_pe(r1, r2, sam=True)
                    assert out[5] is not None and sum(1 for k in out[5] if int(k) != 0xFF) > 0.9 * n
                else:
                    out = ctx.map_se_sliced(r1, [0, 1000, 2500, n], tails=True)
                    assert sum(1 for r in out[4] if r) > 0.8 * n
            finally:
                ctx.close()
            err = capfd.readouterr().err
            if not paired:
                assert "[abm host]" in err, "ABM_TRACE_HOST=1 printed nothing: the check below would be empty"
            lines = [ln for ln in err.splitlines() if "buffer regrown" in ln]
            assert not lines, (paired, lines)
    finally:
        ix.close()


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def _map_bam(chain, args, env_extra):
    env = dict(os.environ, **env_extra)
    # (one name for both runs' files: the header's @PG line carries the command line)
    r = subprocess.run([CLI, "map", "-B", "-timing", "tests/bamrec.json", "-s", "tests/bamrec.mstats", "-o", "tests/bamrec.bam"] + args, cwd=chain, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return (bam_format.bgzf_decompress(open(chain / "tests/bamrec.bam", "rb").read()), open(chain / "tests/bamrec.mstats", "rb").read(),
            json.load(open(chain / "tests/bamrec.json")))


def _device_against_host(chain, args, env, min_records):
    dev = _map_bam(chain, args, dict(env, ABM_CLI_DEVICE_SAM="1"))
    host = _map_bam(chain, args, dict(env, ABM_CLI_DEVICE_SAM="0"))
    assert dev[0] == host[0], "the decompressed BAM streams differ"
    assert dev[1] == host[1], "the statistics differ"
    _, _, recs = bam_format.records_of_stream(dev[0])
    assert len(recs) > min_records
    t1, t0 = dev[2], host[2]
    assert t0["sam_records"]["device"] == 0 and t0["sam_text_by"] == "host"
    assert t1["sam_records"]["device"] > 0 and t1["sam_text_by"] == "device", t1["sam_records"]
    assert t1["sam_records"]["device"] + t1["sam_records"]["host"] == t0["sam_records"]["host"] == len(recs)
    return t1


@pytest.mark.parametrize("flags", [[], ["-a"], ["-R"], ["-A", "-a"]])
def test_cli_single_end_bam_is_byte_identical(chain, flags):
    t1 = _device_against_host(chain, flags + ["-i", "tests/tRex1.idx", "tests/reads_1.fq"], {"ABM_CLI_SLICE_READS": "997"},
                              400 if "-A" in flags else 8000)
    if "-A" not in flags:
        # (the fixture's reads are simulated with 1 % of their bases mutated: a ninth of them align with two indels, five
        # ops or more, and are the host's -- the oracle says 224 of 2,000 such reads)
        assert t1["sam_records"]["device"] > 0.8 * (t1["sam_records"]["device"] + t1["sam_records"]["host"])


def test_cli_odd_reads_bam_is_byte_identical(chain):
    """reads of 44-46 bases, IUPAC letters, CIGARs beyond the slot (the host's records amid the device's) and reads too
    short to map: the file test_sam_text_from_the_device_equals_the_hosts builds"""
    lines = open(chain / "tests/reads_1.fq").read().split("\n")
    rng = random.Random(5)
    for k in range(0, len(lines) - 3, 4):
        seq = lines[k + 1]
        kind = (k // 4) % 7
        if kind == 1:
            seq = seq[:44 + (k // 28) % 3]
        elif kind == 2:
            j = rng.randrange(len(seq))
            seq = seq[:j] + "RYKMSWN"[rng.randrange(7)] + seq[j + 1:]
        elif kind == 3:
            j = rng.randrange(5, len(seq) - 25)
            seq = seq[:j] + seq[j + 2:j + 10] + "A" + seq[j + 10:j + 18] + seq[j + 19:j + 30] + seq[j + 32:]
        elif kind == 4:
            seq = seq[:30]
        lines[k + 1], lines[k + 3] = seq, lines[k + 3][:len(seq)].ljust(len(seq), "B")
    open(chain / "tests/odd_bam.fq", "w").write("\n".join(lines))
    t1 = _device_against_host(chain, ["-i", "tests/tRex1.idx", "tests/odd_bam.fq"], {"ABM_CLI_SLICE_READS": "997"}, 5000)
    assert t1["sam_records"]["host"] > 100, "the reads with five or more ops are the host's"


@pytest.mark.parametrize("flags,reads", [([], "reads_pe"), (["-R"], "reads_rpbat_pe")])
def test_cli_paired_bam_is_byte_identical(chain, flags, reads):
    t1 = _device_against_host(chain, flags + ["-i", "tests/tRex1.idx", f"tests/{reads}_1.fq", f"tests/{reads}_2.fq"],
                              {"ABM_CLI_BATCH_READS": "1000", "ABM_CLI_SLICE_READS": "333"}, 15000)
    assert t1["sam_records"]["device"] > 0.9 * (t1["sam_records"]["device"] + t1["sam_records"]["host"])


# ---- the writer alone ------------------------------------------------------------------------------------------------------
def test_writer_alone_on_fields_mapping_cannot_reach(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "bam_writer_check"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "hip", "bam_writer_check.hip"), "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
