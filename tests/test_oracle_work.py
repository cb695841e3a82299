"""CPU: the oracle's work counters (oracle/abo_map.hpp `Work`), from which bench.py's strict roofline figure is computed
and against which tests/test_gpu_diagnostic_builds.py holds the diagnostic kernels' tallies.

What the counters are, read from oracle/abo_map.cpp:

 * `reads` is counted before anything else (Mapper::map_se: one per read; Mapper::map_pe: two per pair), empty or not;
 * an EMPTY single-end read returns right after that, and a pair of two empty ends leaves every orientation() call before
   its first seed pass: such reads add to `reads` and to no other counter.  A pair with ONE empty end seeds its other end,
   so it does add work;
 * the counters are per-Mapper sums that the C API adds up over its threads, so they cannot depend on the thread count or on
   how a batch is cut -- EXCEPT through reads of 44-46 bases, whose seeds hash past their end into what earlier reads left
   behind (tests/test_oracle_sharding.py): the batches here hold none;
 * `shared_probes3` counts the probes that the two bisections of a 3-letter step make at the same entry in the same round
   (search_probes counts both): additive like the rest, at most half of search_probes, and 0 where nothing is narrowed;
 * `blank_probes2` / `blank_probes3` count bisection probes (first_not) that read a blank genome nibble: an N the indexer did
   not fill (a run of more than 256), or the padding;
 * `pe_full_sets`, `pe_lists_over_512`, `pe_lists_over_4096` and `pe_matings_skipped` tally the paired-end set at its limit of
   32768 entries (abo_map.hpp): what they are on tRex1, on repeat_rich_genome and on the satellite family of
   tests/test_gpu_pe_full_sets.py is pinned below."""
import os

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = [k for k in ob.WORK_KEYS if k != "reads"]


def plus(a, b):
    return {k: a[k] + b[k] for k in ob.WORK_KEYS}


@pytest.fixture(scope="module")
def trex(oracle, trex_index, workdir):
    fa = os.path.join(ROOT, "tests", "golden", "tRex1.fa")
    oracle.simulate(fa, os.path.join(workdir, "work_se"), 1500, single_end=True, seed=21)
    oracle.simulate(fa, os.path.join(workdir, "work_pe"), 600, seed=22)

    def load(name):
        # (no read of 44-46 bases: see above)
        return [r if len(r) >= 50 else "" for r in ob.read_fastq_like_readloader(os.path.join(workdir, name))[1]]

    reads, r1, r2 = load("work_se_1.fq"), load("work_pe_1.fq"), load("work_pe_2.fq")
    # empty reads and pairs, and pairs with one empty end, at known places
    reads[3] = reads[700] = reads[-1] = ""
    r1[5] = r2[5] = ""
    r1[-1] = r2[-1] = ""
    r1[9] = ""
    r2[11] = ""
    oix = oracle.index_load(trex_index)
    yield oix, reads, r1, r2
    oracle.index_free(oix)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_se_work_is_the_same_for_any_thread_count_and_additive(oracle, trex, mode):
    oix, reads, _, _ = trex
    one = oracle.map_se(oix, reads, mode=mode, threads=1)[3]
    eight = oracle.map_se(oix, reads, mode=mode, threads=8)[3]
    assert one == eight
    assert one["reads"] == len(reads)
    assert one["seed_iters"] > 0 and one["candidates"] > 0 and one["words"] >= one["candidates"] and one["set_updates"] > 0
    assert one["aligns"] >= one["aligns_tb"] > 0 and one["dp_cells"] > 0
    cut = (0, 1, 401, 1000, len(reads))  # (uneven parts, one of a single read)
    total = dict.fromkeys(ob.WORK_KEYS, 0)
    for lo, hi in zip(cut, cut[1:]):
        total = plus(total, oracle.map_se(oix, reads[lo:hi], mode=mode, threads=3)[3])
    assert total == one


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pe_work_is_the_same_for_any_thread_count_and_additive(oracle, trex, mode):
    oix, _, r1, r2 = trex
    one = oracle.map_pe(oix, r1, r2, mode=mode, threads=1)[5]
    eight = oracle.map_pe(oix, r1, r2, mode=mode, threads=8)[5]
    assert one == eight
    assert one["reads"] == 2 * len(r1)
    assert one["seed_iters"] > 0 and one["candidates"] > 0 and one["set_updates"] > 0 and one["aligns"] > 0
    cut = (0, 7, 300, len(r1))
    total = dict.fromkeys(ob.WORK_KEYS, 0)
    for lo, hi in zip(cut, cut[1:]):
        total = plus(total, oracle.map_pe(oix, r1[lo:hi], r2[lo:hi], mode=mode, threads=2)[5])
    assert total == one


def test_empty_reads_add_to_reads_only(oracle, trex):
    """the rule stated at the top: empty single-end reads and pairs of two empty ends count as reads and as nothing else;
    a pair with one empty end does seed the other"""
    oix, reads, r1, r2 = trex
    for mode in (0, 2):
        w = oracle.map_se(oix, ["", "", ""], mode=mode)[3]
        assert w["reads"] == 3 and all(w[k] == 0 for k in COUNTERS), w
        w = oracle.map_pe(oix, ["", ""], ["", ""], mode=mode)[5]
        assert w["reads"] == 4 and all(w[k] == 0 for k in COUNTERS), w
        # taking the empty ones out of a batch changes `reads` alone
        full = oracle.map_se(oix, reads, mode=mode, threads=4)[3]
        kept = [r for r in reads if r]
        assert len(kept) <= len(reads) - 3
        less = oracle.map_se(oix, kept, mode=mode, threads=4)[3]
        assert less["reads"] == len(kept) and all(less[k] == full[k] for k in COUNTERS)
        fullp = oracle.map_pe(oix, r1, r2, mode=mode, threads=4)[5]
        keep = [k for k in range(len(r1)) if r1[k] or r2[k]]
        assert len(keep) <= len(r1) - 2
        lessp = oracle.map_pe(oix, [r1[k] for k in keep], [r2[k] for k in keep], mode=mode, threads=4)[5]
        assert lessp["reads"] == 2 * len(keep) and all(lessp[k] == fullp[k] for k in COUNTERS)
        halfp = oracle.map_pe(oix, [r1[0], ""], ["", r2[0]], mode=mode)[5]
        assert halfp["reads"] == 4 and halfp["seed_iters"] > 0


FULL_SET_KEYS = ("pe_full_sets", "pe_lists_over_512", "pe_lists_over_4096", "pe_matings_skipped")


def test_full_set_tallies_on_the_old_fixtures(oracle, trex, workdir):
    """pe_full_sets (PeSet::admit calls that bring a set to 32768 entries), pe_lists_over_512 / _4096 (PeSet::sort_unique
    calls entered with more entries than that) and pe_matings_skipped (orientation calls in which an end's set is full at
    cutoff 0), on the fixtures the suite had before tests/test_gpu_pe_full_sets.py, at default parameters.
    tRex1 never fills a set, never sorts a list of thousands and never skips a mating; a handful of its pairs pass 512
    entries (3, 1 and 4 of these 600 in modes 0, 1 and 2).
    repeat_rich_genome DOES reach all four -- 3000 pairs in mode 0: 7,127,571 admissions into a full set, 438 lists over
    512, 149 over 4096, 38 matings skipped.  Its purine-only and pyrimidine-only tracts are one bucket of the 2-letter
    table that no further letter narrows, so the specific pass scans all of it (seed_passes: `len2 >= spec_len`) whatever
    max_candidates is.  The pairs cut from those tracts are what fills sets there; the satellite family adds the diverged
    family (evictions among distinct distances), the windows wider than a chunk and the filters by end length."""
    oix, reads, r1, r2 = trex
    zero = ("pe_full_sets", "pe_lists_over_4096", "pe_matings_skipped")
    for mode in (0, 1, 2):
        w = oracle.map_pe(oix, r1, r2, mode=mode, threads=8)[5]
        print(f"tRex1 pairs, mode {mode}:", {k: w[k] for k in FULL_SET_KEYS})
        assert w["aligns"] > 0 and all(w[k] == 0 for k in zero), (mode, w)
        assert w["pe_lists_over_512"] < len(r1) // 20, (mode, w)  # (a handful of pairs at most)
        w = oracle.map_se(oix, reads[:200], mode=mode, threads=8)[3]
        assert all(w[k] == 0 for k in FULL_SET_KEYS), (mode, w)  # (single-end has no such set)
    fa = os.path.join(workdir, "work_rep.fa")
    idx = os.path.join(workdir, "work_rep.idx")
    synth.repeat_rich_genome(fa)
    oracle.index_build(fa, idx, threads=4)
    rep = oracle.index_load(idx)
    try:
        a, b = synth.mutated_pairs(fa, 3000, 100, seed=111)
        a, b = synth.trim_like_readloader(a), synth.trim_like_readloader(b)
        for mode in (0, 2):
            w = oracle.map_pe(rep, a, b, mode=mode, threads=8)[5]
            print(f"repeat-rich pairs, mode {mode}:", {k: w[k] for k in FULL_SET_KEYS})
            assert w["aligns"] > 0 and all(w[k] > 0 for k in FULL_SET_KEYS), (mode, w)
            assert w["pe_lists_over_512"] >= w["pe_lists_over_4096"]
    finally:
        oracle.index_free(rep)


def test_full_set_tallies_on_the_satellite_family(oracle, workdir):
    """32 pairs on tests/test_gpu_pe_full_sets.py's genomes at max_candidates 30000.  `near` (2.5 % divergence): sets fill
    and lists of thousands of entries are sorted, no mating is skipped (a set full at cutoff 0 needs 32768 perfect matches);
    `exact` pairs on the family without divergence: every orientation call that finds the family skips its mating, so no
    long list is ever sorted.  Additive over sub-batches and the same for any thread count, like every other tally."""
    from tests.test_gpu_pe_full_sets import COPIES, DIVERGENCE, LEAD, MAXC
    got = {}
    for name, div in (("near", DIVERGENCE), ("exact", 0.0)):
        fa = os.path.join(workdir, f"work_sat_{name}.fa")
        idx = os.path.join(workdir, f"work_sat_{name}.idx")
        lay = synth.satellite_genome(fa, COPIES, 200, div, LEAD, seed=5)
        oracle.index_build(fa, idx, threads=4)
        oix = oracle.index_load(idx)
        try:
            r1, r2 = synth.pairs_on_satellite(lay, fa, 32, 100, seed=7, planted=0.5 if div else 0.0)
            one = oracle.map_pe(oix, r1, r2, mode=0, max_candidates=MAXC, threads=3)[5]
            many = oracle.map_pe(oix, r1, r2, mode=0, max_candidates=MAXC, threads=8)[5]
            assert one == many
            parts = plus(oracle.map_pe(oix, r1[:5], r2[:5], mode=0, max_candidates=MAXC, threads=3)[5],
                         oracle.map_pe(oix, r1[5:], r2[5:], mode=0, max_candidates=MAXC, threads=8)[5])
            assert parts == one
        finally:
            oracle.index_free(oix)
        got[name] = one
    near, exact = got["near"], got["exact"]
    assert near["pe_full_sets"] > 0 and near["pe_lists_over_512"] >= near["pe_lists_over_4096"] > 0 and near["pe_matings_skipped"] == 0, near
    assert exact["pe_full_sets"] > 0 and exact["pe_matings_skipped"] >= 32 and exact["aligns"] == 0, exact
    assert exact["pe_lists_over_512"] == 0, exact


def test_mating_within_max_frag_of_the_first_base_is_reported(oracle, workdir):
    """oracle/README.md, "Hits near the genome's first base": a family whose first copy lies 1000 bases in, mapped with
    max_frag 40000, makes the reference's mating loop take the set's empty entry (position 0) for a partner and align
    before the genome.  The oracle says so -- abo_last_error through the C entry point, a message and status 1 from its
    command line -- and maps the same pairs at the default max_frag, where no hit is in reach of position 0."""
    import subprocess
    from tests import reference_edges as E
    fa = os.path.join(workdir, "work_sat_lead.fa")
    idx = os.path.join(workdir, "work_sat_lead.idx")
    lay = synth.satellite_genome(fa, 2000, 200, 0.025, 1000, seed=5)
    oracle.index_build(fa, idx, threads=4)
    r1, r2 = synth.pairs_on_satellite(lay, fa, 16, 100, seed=7, max_frag=300)
    with pytest.raises(AssertionError, match="raise lead"):
        synth.pairs_on_satellite(lay, fa, 16, 100, seed=7, max_frag=40000)
    oix = oracle.index_load(idx)
    try:
        ok = oracle.map_pe(oix, r1, r2, mode=0, max_candidates=30000, max_frag=300, threads=2)
        assert int((ok[0]["r1"]["pos"] != 0).sum()) > 0
        with pytest.raises(RuntimeError, match="first base"):
            oracle.map_pe(oix, r1, r2, mode=0, max_candidates=30000, max_frag=40000, threads=2)
    finally:
        oracle.index_free(oix)
    E.write_fastq(os.path.join(workdir, "lead_1.fq"), r1)
    E.write_fastq(os.path.join(workdir, "lead_2.fq"), r2)
    r = subprocess.run([ob.CLI, "map", "-c", "30000", "-L", "40000", "-i", idx, "-o", os.path.join(workdir, "lead.sam"),
                        os.path.join(workdir, "lead_1.fq"), os.path.join(workdir, "lead_2.fq")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 1 and "first base" in r.stdout, (r.returncode, r.stdout)


def family_genome_without_n(path, seed=31, chrom_len=150_000, copies=200):
    """random sequence with one 300-base repeat family at 2 % divergence, its copies away from the chromosome's ends, and
    not one N: buckets big enough to be narrowed, no blank letter for a probe to read"""
    rng = np.random.default_rng(seed)
    seq = synth.ACGT[rng.integers(0, 4, chrom_len)].copy()
    fam = synth._n_run_family(rng, 300, 10)  # (inner repeats: every copy's kept positions fall into a few buckets)
    for at in rng.integers(5000, chrom_len - 5000, copies):
        piece = fam.copy()
        m = rng.random(300) < 0.02
        piece[m] = synth.ACGT[rng.integers(0, 4, int(m.sum()))]
        seq[at:at + 300] = piece
    with open(path, "wb") as f:
        f.write(b">fam\n" + b"\n".join(bytes(seq[i:i + 70]) for i in range(0, chrom_len, 70)) + b"\n")


def test_blank_probes_need_an_unfilled_n_run(oracle, workdir):
    """zero on a genome without any N whose big buckets lie away from its ends (no probe reaches the padding); non-zero on
    both kinds of table on the bed of tests/test_gpu_narrowing_at_n_runs.py, whose repeat copies are cut short by runs
    of 300 N"""
    fa = os.path.join(workdir, "work_no_n.fa")
    idx = os.path.join(workdir, "work_no_n.idx")
    family_genome_without_n(fa)
    oracle.index_build(fa, idx, threads=4)
    oix = oracle.index_load(idx)
    try:
        rd = synth.trim_like_readloader(synth.mutated_reads(fa, 800, 100, seed=7, n_frac=0.0))
        p1, p2 = synth.mutated_pairs(fa, 300, 100, seed=8)
        for c in (100, 20):
            w = oracle.map_se(oix, rd, mode=0, max_candidates=c, threads=4)[3]
            wp = oracle.map_pe(oix, synth.trim_like_readloader(p1), synth.trim_like_readloader(p2), mode=0, max_candidates=c, threads=4)[5]
            assert w["search_probes"] > 0 and wp["search_probes"] > 0, "nothing was narrowed: the zeros below would say nothing"
            assert w["blank_probes2"] == w["blank_probes3"] == wp["blank_probes2"] == wp["blank_probes3"] == 0, (c, w, wp)
    finally:
        oracle.index_free(oix)
    fa = os.path.join(workdir, "work_n_runs.fa")
    idx = os.path.join(workdir, "work_n_runs.idx")
    lay = synth.repeats_against_n_runs(fa)
    oracle.index_build(fa, idx, threads=4)
    bed = oracle.index_load(idx)
    try:
        rd = synth.trim_like_readloader(synth.reads_against_n_runs(lay, fa, 100, seed=1100, mode=0))
        w = oracle.map_se(bed, rd, mode=0, threads=4)[3]
        assert w["blank_probes2"] > 0 and w["blank_probes3"] > 0, w
        assert w["blank_probes2"] + w["blank_probes3"] <= w["search_probes"]
        assert 0 < 2 * w["shared_probes3"] <= w["search_probes"], w
        p1, p2 = synth.pairs_against_n_runs(lay, fa, 100, seed=2100)
        wp = oracle.map_pe(bed, synth.trim_like_readloader(p1), synth.trim_like_readloader(p2), mode=0, threads=4)[5]
        assert wp["blank_probes2"] > 0 and wp["blank_probes3"] > 0, wp
    finally:
        oracle.index_free(bed)
