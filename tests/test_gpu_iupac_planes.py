"""GPU parity of abm_index_set_iupac_planes: a genome with IUPAC letters keeps its bit planes, window records, direct
narrowing and device-written text; the 4096-base chunks (nmap) and the records' stretches that hold such a letter are marked
as blank nibbles are, and the filters redo marked candidates on the nibble array -- on the records BEFORE the cutoff test (a
multi-bit nibble can match where its arbitrary plane code does not: the planes' distance is no lower bound there), and with
their own largest prefix sum (such a letter can make a word's share negative, and admission follows every prefix sum:
full_compare, src/abismal.cpp:1105-1122).  Results equal the oracle's bit for bit on every path; the option off, or a genome
without such letters, is today's behaviour.

Genomes: synth.repeat_rich_genome(2 x 400 kbp) with 40 letters per chromosome (sparse: most chunks unflagged), 3000 (every
chunk flagged) and none, and tests/iupac_fixture.hand_built_genome.  Liveness is computed in numpy from the FASTA
(tests/iupac_fixture.py) before anything is compared.

Seeded defects -- each built once in a scratch copy of the tree and run on the GPU against this module (the hand-built
genome's 100-base cases) and tests/hip/iupac_marks_check.hip; all four are caught:

 1. on the records, the flag is consulted only for candidates already within the cutoff: test_se_equals_the_oracle_on_every_path
    [hand-100-0] and [hand-100-2] ("records for 108 ...: 36 of 959 reads differ; first: (711, 'pos', 0, 82767)": the 36
    windows of kind (a) stay unmapped) and all three test_pe_equals_the_oracle_on_every_path[hand-100-*] ("36 of 617 pairs
    differ ... 'pair presence', False, True").
 2. `hma = ha` kept after a redo: test_se_equals_the_oracle_on_every_path[hand-100-0] ("records for 0 ...: 1 of 959 reads
    differ; first: (509, 'pos', 98896, 0)") and test_pe_equals_the_oracle_on_every_path[hand-100-2] ("1 of 617 pairs
    differ").  One read, not the thirty of kind (b): admitted with d = 6, the other windows' alignments over 48 mismatching
    bases are then rejected all the same.
 3. nmap marks for multi-bit nibbles made without the reach: iupac_marks_check ("chunk 4 holds a position with a marked nibble
    within 512 bases and is not flagged (nmap incomplete)") and
    test_sparse_genome_has_reads_on_both_sides_and_the_chunk_count_is_the_rule (plane_chunks() on the sparse genome); the
    hand-built genome's single-end parity cases passed with it.
 4. the record flag set from blanks only: iupac_marks_check ("entry 0 at 8274 has spare bits 0 (low) 0 (high); its stretch
    holds a marked nibble") and all six test_pe_equals_the_oracle_on_every_path[dense-100-*] / [hand-100-*] ("records for
    108 ...: 47 of 700 pairs differ", "36 of 617 pairs differ").

 5. (from review) the record flag without the 15 bases after the stretch, where a multi-bit nibble lies under the 0xF padding
    of a window's last word: iupac_marks_check ("3 blocks: entry 3 at 8083 has spare bits 0 (low) 0 (high); its stretch holds a
    marked nibble").  Not visible to parity: 24 windows planted for it (plane distance L / 10 + 1 and + 2, d = dmax = L / 10 by
    the letter alone, whole seeds at offsets 0 ... 3 only) are left unmapped by the oracle -- the final alignment gets no credit
    from the padding -- and a candidate dropped by the specific pass comes back in the sensitive one, whose cutoff is
    0.4 L until the set is full.

Times (MI355X): the module 170 s -- pairs 6-10 s a case (twelve device configurations and two oracle runs each), single-end
2-4 s, each of the nineteen command-line cases 6 s (a process, a context and the records each)."""
import json
import os

import numpy as np
import pytest

from tests import iupac_fixture as F
from tests import reference_edges as E
from tests import synth
from tests.test_gpu_diagnostic_builds import same_bytes, stamped
from tests.test_gpu_pe_parity import compare_pe
from tests.test_gpu_pe_sam_text import check_text, mapped_twice, same_results
from tests.test_gpu_se_parity import compare_se

pytestmark = pytest.mark.gpu

RECORDS = ((0, 0), (108, 108), (172, 172))  # (asked for, serves): none, three blocks, five blocks
DIRECT = (0, 64)
MAX_CANDIDATES = (100, 20)
N_READS, N_PAIRS = 2000, 700
GENOMES = ("sparse", "dense", "hand")


class Bed:
    def __init__(self, oracle, workdir, name):
        import abismal_amd as A
        self.oracle, self.name = oracle, name
        self.fa = os.path.join(workdir, f"iupac_planes_{name}.fa")
        self.idx = os.path.join(workdir, f"iupac_planes_{name}.idx")
        self.planted = None
        if name == "hand":
            self.planted = F.hand_built_genome(self.fa)
        else:
            synth.repeat_rich_genome(self.fa, seed=31, n_chroms=2, chrom_len=400_000, iupac={"sparse": 40, "dense": 3000, "none": 0}[name])
        A.index_build(self.fa, self.idx, 8)
        self.oix = oracle.index_load(self.idx)
        self.nib, self.starts = F.genome_nibbles(self.fa)
        self._se, self._pe, self._ose, self._ope, self._ctx = {}, {}, {}, {}, {}

    def close(self):
        for ix, ctx in self._ctx.values():
            ctx.close()
            ix.close()
        self.oracle.index_free(self.oix)

    def reads(self, L, mode):
        if (L, mode) not in self._se:
            r = synth.mutated_reads(self.fa, N_READS, L, seed=100 + L + mode, pbat_frac=0.5 if mode == 2 else 0.0)
            if self.planted:
                r = r[:600] + [p["seq"] for p in self.planted if p["L"] == L]
            self._se[L, mode] = synth.trim_like_readloader(r)
        return self._se[L, mode]

    def pairs(self, L, mode):
        if (L, mode) not in self._pe:
            r1, r2 = synth.mutated_pairs(self.fa, N_PAIRS, L, seed=200 + L)
            r1, r2 = [x.decode() for x in r1], [x.decode() for x in r2]
            if self.planted:
                p1, p2 = F.mates_for(self.fa, [p for p in self.planted if p["L"] == L])
                r1, r2 = r1[:400] + p1, r2[:400] + p2
            r1, r2 = synth.trim_like_readloader(r1), synth.trim_like_readloader(r2)
            if mode == 1:
                r1, r2 = r2, r1
            elif mode == 2:
                for k in range(1, len(r1), 2):
                    r1[k], r2[k] = r2[k], r1[k]
            self._pe[L, mode] = (r1, r2)
        return self._pe[L, mode]

    def expected_se(self, L, mode, c):
        if (L, mode, c) not in self._ose:
            out = self.oracle.map_se(self.oix, self.reads(L, mode), mode=mode, threads=8, max_candidates=c)
            assert (out[0]["pos"] != 0).mean() > 0.5 and out[3]["candidates"] > 0
            self._ose[L, mode, c] = out
        return self._ose[L, mode, c]

    def expected_pe(self, L, mode, c):
        if (L, mode, c) not in self._ope:
            r1, r2 = self.pairs(L, mode)
            out = self.oracle.map_pe(self.oix, r1, r2, mode=mode, threads=8, max_candidates=c)
            assert (out[0]["r1"]["pos"] != 0).mean() > 0.5
            self._ope[L, mode, c] = out
        return self._ope[L, mode, c]

    def ctx(self, asked, serves, planes=True):
        """the context with records asked for `asked` bases, its path asserted; planes=False: the option left off"""
        import abismal_amd as A
        if (asked, planes) not in self._ctx:
            ix = A.Index(self.idx, window_records=asked, iupac_planes=True if planes else None)
            self._ctx[asked, planes] = (ix, A.Context(ix, 0))
        ix, ctx = self._ctx[asked, planes]
        if self.name != "none":
            assert ctx.filter_on_planes() == planes, "filter_on_planes"
            assert ctx.window_records() == (serves if planes else 0), "window records"
            assert ctx.seed_extension()[:2] == (0, 0), "a genome with IUPAC letters gets no seed-extension tables"
        return ix, ctx


_beds = {}


@pytest.fixture(scope="module")
def beds(oracle, workdir):
    def get(name):
        if name not in _beds:
            _beds[name] = Bed(oracle, workdir, name)
        return _beds[name]
    yield get
    for b in _beds.values():
        b.close()
    _beds.clear()


# ---- liveness, on the CPU ------------------------------------------------------------------------------------------------
def test_hand_built_windows_are_what_they_are_planted_for(beds):
    """numpy, from the FASTA: at least 20 windows each whose distance is within L / 10 only because ambiguity letters match
    (plane distance above 0.4 L, the sensitive pass's widest cutoff), and whose largest prefix sum is above 0.4 L while the
    total is within L / 10; the oracle maps the first kind where they were planted and none of the second kind"""
    bed = beds("hand")
    base = bed.starts[0]
    kinds = {"matches": 0, "prefix": 0}
    for p in bed.planted:
        if p["kind"] not in kinds:
            continue
        L = p["L"]
        d, dmax, plane = F.distances(bed.nib, base + p["at"], p["seq"])
        if p["kind"] == "matches":
            # (d may be below 0: the K's under the 0xF padding of the read's last word count -1 each, like any match on two bits)
            assert d <= L // 10 and dmax <= L // 10 and plane > 0.4 * L, (p, d, dmax, plane)
        else:
            assert 0 <= d <= L // 10 and dmax > 0.4 * L, (p, d, dmax)
        kinds[p["kind"]] += 1
    print(kinds)
    assert min(kinds.values()) >= 20, kinds
    for L in (100, 150):
        reads = bed.reads(L, 0)
        o_res = bed.expected_se(L, 0, 100)[0]
        planted = [p for p in bed.planted if p["L"] == L]
        hits = o_res[len(reads) - len(planted):]
        at_a = sum(1 for p, h in zip(planted, hits) if p["kind"] == "matches" and abs(int(h["pos"]) - (base + p["at"])) <= 8)
        # the same three figures at the positions the oracle itself reports, in the orientation it reports (a hit's position
        # is its alignment's first base: the window's, unless the alignment clipped the read's start)
        own_a = 0
        for p, h in zip(planted, hits):
            if p["kind"] == "matches" and int(h["pos"]) != 0:
                rc, a_rich = bool(int(h["flags"]) & 0x10), bool(int(h["flags"]) & 0x1000)
                d, dmax, plane = F.distances(bed.nib, int(h["pos"]), p["seq"], rc=rc, g_to_a=rc != a_rich)
                own_a += d <= L // 10 and dmax <= L // 10 and plane > 0.4 * L
        print(f"L {L}: at the oracle's own positions {own_a} windows are within L / 10 with a plane distance above 0.4 L")
        assert own_a >= 20
        at_b = sum(1 for p, h in zip(planted, hits) if p["kind"] == "prefix" and int(h["pos"]) != 0)
        print(f"L {L}: the oracle maps {at_a} windows of kind (a) where planted and {at_b} of kind (b) anywhere")
        assert at_a >= 20 and at_b == 0


def test_sparse_genome_has_reads_on_both_sides_and_the_chunk_count_is_the_rule(beds):
    """K = 40: at least a fifth of the mapped reads start in flagged chunks and a fifth in unflagged ones; plane_chunks()
    equals the numpy count exactly, on every genome"""
    for name in GENOMES:
        bed = beds(name)
        n_chunks, flag = F.flagged_chunks(bed.nib)
        ix, ctx = bed.ctx(172, 172)
        print(name, ctx.plane_chunks(), (n_chunks, int(flag.sum())))
        assert ctx.plane_chunks() == (n_chunks, int(flag.sum())), name
        ix0, ctx0 = bed.ctx(172, 172, planes=False)
        assert ctx0.plane_chunks() == (0, 0)
        if name == "sparse":
            pos = bed.expected_se(100, 0, 100)[0]["pos"]
            pos = pos[pos != 0].astype(np.int64)
            in_flagged = float(flag[pos >> F.CHUNK_BITS].mean())
            print(f"sparse: {in_flagged:.3f} of {len(pos)} mapped reads start in a flagged chunk")
            assert 0.2 <= in_flagged <= 0.8
        if name == "dense":
            assert flag.all()


# ---- parity with the oracle ----------------------------------------------------------------------------------------------
def configurations():
    for asked, serves in RECORDS:
        for direct in DIRECT:
            for c in MAX_CANDIDATES:
                yield asked, serves, direct, c


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("L", [100, 150])
@pytest.mark.parametrize("name", GENOMES)
def test_se_equals_the_oracle_on_every_path(beds, name, L, mode):
    """records for 0 / 108 / 172 bases (100-base reads: bit planes with two-lane groups, three-block records, the two-lane
    build on five-block records; 150: four-lane groups, again the planes -- 108 does not serve them -- and five-block
    records), direct narrowing never and from 64 entries, -c 100 and 20"""
    import abismal_amd as A
    bed = beds(name)
    reads = bed.reads(L, mode)
    for asked, serves, direct, c in configurations():
        o_res, o_cig, o_n, _ = bed.expected_se(L, mode, c)
        ix, ctx = bed.ctx(asked, serves)
        ix.set_direct_narrowing(direct)
        res, cig, off = ctx.map_se(reads, mode=mode, params=A.Params(max_candidates=c))
        compare_se(res, cig, off, o_res, o_cig, o_n, reads, f"{name} SE {L} mode {mode}, records for {serves}, direct from {direct}, -c {c}")


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("L", [100, 150])
@pytest.mark.parametrize("name", GENOMES)
def test_pe_equals_the_oracle_on_every_path(beds, name, L, mode):
    import abismal_amd as A
    bed = beds(name)
    r1, r2 = bed.pairs(L, mode)
    for asked, serves, direct, c in configurations():
        orc = bed.expected_pe(L, mode, c)
        ix, ctx = bed.ctx(asked, serves)
        ix.set_direct_narrowing(direct)
        compare_pe(ctx.map_pe(r1, r2, mode=mode, params=A.Params(max_candidates=c)), orc,
                   f"{name} PE 2 x {L} mode {mode}, records for {serves}, direct from {direct}, -c {c}")


@pytest.mark.parametrize("name", GENOMES)
def test_ragged_batches_from_44_bases(beds, name):
    bed = beds(name)
    rng = np.random.default_rng(9)
    pool = bed.reads(150, 0)
    reads = synth.trim_like_readloader([r[: int(rng.integers(44, 151))] for r in pool[:-1]] + [synth.mutated_reads(bed.fa, 1, 150, seed=1, n_frac=0.0)[0]])
    assert max(len(r) for r in reads) == 150
    # (44-46 bases: such reads hash past their end, into what the reads before them left behind -- in input order)
    o_res, o_cig, o_n, _ = bed.oracle.map_se(bed.oix, reads, mode=0, threads=1)
    p1, p2 = bed.pairs(150, 0)
    r1, r2 = synth.cut_pairs_ragged(p1, p2, rng, 44, 150)
    r1, r2 = synth.trim_like_readloader(r1), synth.trim_like_readloader(r2)
    orc = bed.oracle.map_pe(bed.oix, r1, r2, mode=0, threads=1)
    for asked, serves in RECORDS:
        ix, ctx = bed.ctx(asked, serves)
        ix.set_direct_narrowing(64)
        res, cig, off = ctx.map_se(reads, mode=0)
        compare_se(res, cig, off, o_res, o_cig, o_n, reads, f"{name} ragged SE, records for {serves}")
        compare_pe(ctx.map_pe(r1, r2, mode=0), orc, f"{name} ragged PE, records for {serves}")


@pytest.mark.parametrize("name", ["sparse", "hand"])
def test_device_written_sam_text(beds, name):
    """text on and off: results unchanged; the pairs' text equals tests/sam_format.py byte for byte; the single-end text is the
    same from the record-fed build and from the planes"""
    bed = beds(name)
    reads = bed.reads(100, 0)
    r1, r2 = bed.pairs(100, 0)
    orc = bed.expected_pe(100, 0, 100)
    se_text = {}
    for asked, serves in ((172, 172), (0, 0)):
        ix, ctx = bed.ctx(asked, serves)
        ix.set_direct_narrowing(64)
        plain, text = mapped_twice(ctx, r1, r2, 0, False)
        same_results(plain, text, f"{name} PE text, records for {serves}")
        compare_pe(plain, orc, f"{name} PE text off, records for {serves}")
        check_text(ix, r1, r2, text, False, f"{name} PE text, records for {serves}", min_device=0.9)
        cuts = [0, 300, len(reads)]
        off_run = ctx.map_se_sliced(reads, cuts, mode=0)[:3]
        ctx.set_sam_tails(True)
        try:
            on_run = ctx.map_se_sliced(reads, cuts, mode=0, tails=True)
        finally:
            ctx.set_sam_tails(False)
        same_bytes(off_run, on_run[:3], f"{name} SE text on and off")
        o_res, o_cig, o_n, _ = bed.expected_se(100, 0, 100)
        compare_se(*on_run[:3], o_res, o_cig, o_n, reads, f"{name} SE with text, records for {serves}")
        written = [t for t in on_run[4] if t]
        assert len(written) > 0.5 * sum(1 for r in reads if r), "the launch wrote its reads' text"
        se_text[serves] = on_run[4]
    assert se_text[172] == se_text[0], "single-end text differs between the record-fed build and the planes"


@pytest.mark.parametrize("name", ["sparse", "hand"])
def test_diagnostic_builds_equal_the_production_builds(beds, name):
    bed = beds(name)
    reads = bed.reads(100, 2)
    r1, r2 = bed.pairs(150, 0)
    for asked, serves in ((172, 172), (0, 0)):
        ix, ctx = bed.ctx(asked, serves)
        ix.set_direct_narrowing(64)
        plain = ctx.map_se(reads, mode=2)
        diag, tiers = stamped(ctx, lambda: ctx.map_se(reads, mode=2))
        same_bytes(plain, diag, f"{name} SE, records for {serves}")
        assert tiers[0]["cyc_total"] > 0
        plain = ctx.map_pe(r1, r2, mode=0)
        diag, tiers = stamped(ctx, lambda: ctx.map_pe(r1, r2, mode=0))
        same_bytes(plain, diag, f"{name} PE, records for {serves}")
        assert tiers[0]["cyc_total"] > 0


# ---- the switch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "hand"])
def test_without_the_option_nothing_changes(beds, name):
    """the same index opened without the option: no planes, no records, and the same results"""
    bed = beds(name)
    reads = bed.reads(100, 0)
    r1, r2 = bed.pairs(100, 0)
    ix0, ctx0 = bed.ctx(172, 172, planes=False)
    assert ctx0.filter_on_planes() == 0 and ctx0.window_records() == 0 and ctx0.plane_chunks() == (0, 0)
    ix1, ctx1 = bed.ctx(172, 172)
    same_bytes(ctx0.map_se(reads, mode=0), ctx1.map_se(reads, mode=0), f"{name} SE, option off and on")
    same_bytes(ctx0.map_pe(r1, r2, mode=0)[:5], ctx1.map_pe(r1, r2, mode=0)[:5], f"{name} PE, option off and on")
    o_res, o_cig, o_n, _ = bed.expected_se(100, 0, 100)
    compare_se(*ctx0.map_se(reads, mode=0), o_res, o_cig, o_n, reads, f"{name} SE, option off")


def test_the_option_is_a_no_op_without_ambiguity_letters(beds):
    bed = beds("none")
    reads = bed.reads(100, 0)
    r1, r2 = bed.pairs(100, 0)
    ix0, ctx0 = bed.ctx(172, 172, planes=False)
    ix1, ctx1 = bed.ctx(172, 172)
    n_chunks, flag = F.flagged_chunks(bed.nib)
    for ctx in (ctx0, ctx1):
        assert ctx.filter_on_planes() and ctx.window_records() == 172 and ctx.seed_extension()[:2] == (2, 1)
        assert ctx.plane_chunks() == (n_chunks, int(flag.sum()))
    same_bytes(ctx0.map_se(reads, mode=0), ctx1.map_se(reads, mode=0), "no letters, SE")
    same_bytes(ctx0.map_pe(r1, r2, mode=0)[:5], ctx1.map_pe(r1, r2, mode=0)[:5], "no letters, PE")
    o_res, o_cig, o_n, _ = bed.expected_se(100, 0, 100)
    compare_se(*ctx1.map_se(reads, mode=0), o_res, o_cig, o_n, reads, "no letters, option on")


def test_the_setter_must_precede_the_first_context(beds):
    import abismal_amd as A
    bed = beds("sparse")
    ix, ctx = bed.ctx(172, 172)
    with pytest.raises(A.AbismalAmdError):
        ix.set_iupac_planes(False)


# ---- the command line ----------------------------------------------------------------------------------------------------
REP_CASES = [c["name"] for c in E.CASES if c["index"] == "rep" and not c.get("refused")]


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("iupac_planes_cli"))
    made = E.make_inputs(wd)
    man = E.load_manifest()
    idx = E.build_index("product", "rep", wd, os.path.join(wd, "product_rep.idx"), timeout=300)
    return {"wd": wd, "made": made, "entries": {e["name"]: e for e in man["cases"]}, "idx": idx}


@pytest.mark.parametrize("name", REP_CASES)
def test_map_with_iupac_planes_reproduces_the_reference(matrix, name):
    """the reference edge matrix's cases on its `rep` genome (3000 IUPAC letters per chromosome) through `abismal-amd map
    -iupac-planes`: SAM body and statistics equal what the reference binary answered (tests/golden/reference_edges.json); the
    timing JSON says how much of the genome goes the slow way"""
    import subprocess
    case = next(c for c in E.CASES if c["name"] == name)
    entry = matrix["entries"][name]
    assert not E.stale_inputs(entry, matrix["made"])
    prefix = os.path.join(matrix["wd"], f"product_{name}")
    timing = prefix + ".timing.json"
    try:
        r = E.run_map("product", case, matrix["wd"], matrix["idx"], prefix, extra=["-iupac-planes", "-timing", timing], timeout=180)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"abismal-amd map hung on {name}: {e}", returncode=3)
    if r.returncode < 0 or r.returncode >= 128:
        pytest.exit(f"abismal-amd map died on {name} (status {r.returncode}):\n{r.stdout}", returncode=3)
    assert r.returncode == 0, r.stdout
    got, want = E.digest(prefix), {k: entry[k] for k in ("records", "sam_md5", "stats_md5")}
    assert got == want, f"{name}: {got} != recorded {want}"
    t = json.load(open(timing))
    assert t["plane_chunks"] > 0 and 0 < t["plane_chunks_flagged"] <= t["plane_chunks"], t
    assert t["window_records_serve_reads_up_to"] > 0, "with the planes come the window records"


def test_map_without_the_switch_reports_no_planes(matrix):
    case = next(c for c in E.CASES if c["name"] == "se_default")
    prefix = os.path.join(matrix["wd"], "product_se_default_off")
    timing = prefix + ".timing.json"
    r = E.run_map("product", case, matrix["wd"], matrix["idx"], prefix, extra=["-timing", timing], timeout=180)
    assert r.returncode == 0, r.stdout
    t = json.load(open(timing))
    assert t["plane_chunks"] == 0 and t["plane_chunks_flagged"] == 0 and t["window_records_serve_reads_up_to"] == 0
    env = dict(os.environ, ABM_CLI_IUPAC_PLANES="1")
    r = E.run_map("product", case, matrix["wd"], matrix["idx"], prefix, extra=["-timing", timing], env=env, timeout=180)
    assert r.returncode == 0, r.stdout
    assert json.load(open(timing))["plane_chunks_flagged"] > 0
