"""The diagnostic builds of the mapping kernels (abm_ctx_set_phase_stamps): their results, their work tallies, their cycle
stamps and the launch timers -- everything bench.py's roofline counts, phase shares and read-by-read comparison rest on.

Diagnostic builds (timed = true), as se_select / pe_select (abm_kernel_form.hpp) choose them, by the fields that tell them
apart, the case that runs each and what proves it ran.  (tests/test_gpu_kernel_forms.py asserts the builds themselves, as
the context reports them; the proofs here are the tallies' own.)
Every case maps its batch with the stamps off and on on one context, compares the two runs byte for byte and both with
the oracle (same_bytes, compare_se / compare_pe), and asserts that the tallies carry cycles (`phase_cycles` total for single-end,
`cyc_total` of the tier for pairs).

SeForm, timed, not is_long -- three:
  coop, rec                         record-fed      test_se_results[rep-records-*, unique-records-*]: window_records() != 0,
                                                    window_cache_hits == 0 (this build alone has no position cache)
  coop, no rec                      bit planes      test_se_results[rep-planes-*, unique-planes-*]: filter_on_planes(),
                                                    window_records() == 0, window_cache_hits > 0 on rep
  no coop                           nibble array    test_se_results[iupac-*]: filter_on_planes() == 0; and
                                                    test_read_words_per_window[460] (reads beyond 448 bases)
PeForm, timed, phase whole -- five.  (Tier 1, not big, has TWO filter forms, not three: pe_select takes the record-fed
build for big and for the seed kernel only, so an index with records runs tier 1 unsplit on the planes.)
  not big, coop                     tier 1, planes  test_pe_results[rep-planes-unsplit-*, rep-records-unsplit-*]: no pair routed,
                                                    tier 1's cyc_total and seed_offsets > 0
  not big, no coop                  tier 1, nibbles test_pe_results[iupac-unsplit-*]: the same, filter_on_planes() == 0
  big, coop, rec                    tier 2, records test_pe_results[rep-records-*]: tier 2's seed_offsets > 0 (only the
                                                    whole-pair kernel seeds in tier 2), window_records() == 172
  big, coop, no rec                 tier 2, planes  test_pe_results[rep-planes-*]: tier 2's seed_offsets > 0
  big, no coop                      tier 2, nibbles test_pe_results[iupac-*]: tier 2's seed_offsets > 0
PeForm, timed, phase seed -- three (the split routes):
  coop, rec                         records         test_pe_results[rep-records-split*]: routes add up to the batch
  coop, no rec                      planes          test_pe_results[rep-planes-split*]: the same
  no coop                           nibbles         test_pe_results[iupac-split*]: the same
PeForm, timed, phase mate -- two (neither filters, so one build serves every index):
  not big                           small lists     test_pe_results[*-split*]: mated_from_lds > 0, tier 1's alignments > 0
  big                               lists in memory test_pe_results[*-split_stage_16384-*]: mated_from_device_memory > 0 and
                                                    tier 2's alignments > 0
Modes: single-end 0, 1 and 2 and paired 0, 1 and 2 each occur at least twice in the parameter lists below.

What "byte for byte" covers: the host entry points return hits, pair records, fallback hits and CIGARs as a compact blob
with offsets -- the blob is the device's CIGAR counts, slots and long-CIGAR arena put together, and a status word with
ABM_STATUS_CIGAR_OVERFLOW / _SET_OVERFLOW makes the call map again or fail -- so equal blobs and offsets are equal counts,
slots and arena.  (The raw arena is not comparable between two runs of ANY build: waves take their room in it with an
atomic add, in whatever order they finish, and a slot's first word holds where.)

Tally relations (section "tallies"): each test's docstring derives its relation from seed_pass (abm_seed.hpp) and
Impl::seed_passes (oracle/abo_map.cpp) and says whether it is exact or a two-sided bound."""
import os
import time

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_pe_parity import compare_pe
from tests.test_gpu_pe_split import FORMS
from tests.test_gpu_se_parity import compare_se

pytestmark = pytest.mark.gpu

FORM = dict(FORMS)
PE_FORMS = ("unsplit", "split", "split_stage_16384")
SEED_KEYS = ("seed_offsets", "search_probes", "candidates", "set_updates")
COUNT_KEYS = ("seed_offsets", "search_probes", "candidates", "index_run_lines", "set_updates", "alignments", "window_cache_hits")
PE_CYCLE_PARTS = ("cyc_probe_narrow", "cyc_gather_hamming", "cyc_replay", "cyc_sort_unique", "cyc_score_pairable", "cyc_mate",
                  "cyc_best_single", "cyc_se_fallback")
TIER1_CAP = 256  # abismal_amd.h: "tier 1 (sets of up to 256 entries)"
LDS_READ_LEN = 1024  # abismal_amd.h: reads of up to 1024 bases are mapped by a batch's main launch


def no_ghost_reads(reads):
    """reads of 44-46 bases hash past their end into what the reads before them left behind (tests/test_oracle_sharding.py):
    their work depends on the batch they are in, which the tallies of sub-batches here must not"""
    return [r if len(r) >= 50 else "" for r in synth.trim_like_readloader(reads)]


class Bed:
    """a genome, its index, reads and pairs cut from it, the oracle's answers (computed once each) and one context per
    (seed-extension letters, window records, direct narrowing)"""

    def __init__(self, oracle, workdir, name, make):
        import abismal_amd as A
        self.oracle, self.name = oracle, name
        self.fa = os.path.join(workdir, f"diag_{name}.fa")
        self.idx = os.path.join(workdir, f"diag_{name}.idx")
        make(self.fa)
        A.index_build(self.fa, self.idx, 8)
        self.oix = oracle.index_load(self.idx)
        self._reads, self._pairs, self._ose, self._ope, self._ctx = {}, {}, {}, {}, {}

    def close(self):
        for ix, ctx in self._ctx.values():
            ctx.close()
            ix.close()
        self.oracle.index_free(self.oix)

    def reads(self, mode, L=100, n=2000, uniform=False):
        """mode 0: C->T reads, 1: G->A, 2: half and half; uniform: only reads of exactly L bases"""
        key = (mode, L, n, uniform)
        if key not in self._reads:
            rd = no_ghost_reads(synth.mutated_reads(self.fa, n, L, seed=40 + L + mode, pbat_frac=(0.0, 1.0, 0.5)[mode]))
            self._reads[key] = [r for r in rd if len(r) == L] if uniform else rd
        return self._reads[key]

    def pairs(self, mode, L=100, n=1000):
        """mode 1 (PBAT): the A-rich end comes first; mode 2 (random PBAT): in every other pair"""
        if (mode, L, n) not in self._pairs:
            r1, r2 = synth.mutated_pairs(self.fa, n, L, seed=60 + L)
            r1, r2 = no_ghost_reads(r1), no_ghost_reads(r2)
            if mode == 1:
                r1, r2 = r2, r1
            elif mode == 2:
                for k in range(1, n, 2):
                    r1[k], r2[k] = r2[k], r1[k]
            self._pairs[mode, L, n] = (r1, r2)
        return self._pairs[mode, L, n]

    def expected_se(self, reads, mode, tag):
        if tag not in self._ose:
            self._ose[tag] = self.oracle.map_se(self.oix, reads, mode=mode, threads=8)
        return self._ose[tag]

    def expected_pe(self, r1, r2, mode, tag):
        if tag not in self._ope:
            self._ope[tag] = self.oracle.map_pe(self.oix, r1, r2, mode=mode, threads=8)
        return self._ope[tag]

    def ctx(self, letters=(0, 0), records=0, direct=0):
        """direct: 0 = never narrow directly, None = the library's default threshold"""
        import abismal_amd as A
        key = (letters, records, direct)
        if key not in self._ctx:
            ix = A.Index(self.idx, seed_extension=letters, window_records=records)
            if direct is not None:
                ix.set_direct_narrowing(direct)
            self._ctx[key] = (ix, A.Context(ix, 0))
        ix, ctx = self._ctx[key]
        assert ctx.seed_extension()[:2] == letters and (ctx.window_records() != 0) == (records != 0)
        ctx.set_pe_split(-1)
        ctx.set_phase_stamps(False)
        ctx.take_work()
        ctx.pe_split_stats()
        return ctx


def unique_genome(path, seed=9, n_chroms=2, chrom_len=300_000):
    """random sequence: no repeats to speak of, no N, no IUPAC letters"""
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        for c in range(n_chroms):
            seq = synth.ACGT[rng.integers(0, 4, chrom_len)]
            f.write(b">u%d\n" % (c + 1))
            f.write(b"\n".join(bytes(seq[i:i + 70]) for i in range(0, chrom_len, 70)) + b"\n")


@pytest.fixture(scope="module")
def beds(oracle, workdir):
    made = {}

    def get(name):
        if name not in made:
            make = {"unique": unique_genome,
                    "rep": lambda p: synth.repeat_rich_genome(p, n_chroms=2, chrom_len=400_000),
                    "iupac": lambda p: synth.repeat_rich_genome(p, n_chroms=2, chrom_len=400_000, iupac=3000)}[name]
            made[name] = Bed(oracle, workdir, name, make)
        return made[name]

    yield get
    for b in made.values():
        b.close()


def stamped(ctx, fn):
    """fn() under the diagnostic builds; (its value, take_work_tiers() of exactly that work)"""
    ctx.take_work()
    ctx.set_phase_stamps(True)
    try:
        out = fn()
        tiers = ctx.take_work_tiers()
    finally:
        ctx.set_phase_stamps(False)
    return out, tiers


def se_tally(ctx, reads, mode):
    """take_work() of one stamped single-end call"""
    ctx.take_work()
    ctx.set_phase_stamps(True)
    try:
        ctx.map_se(reads, mode=mode)
        return ctx.take_work()
    finally:
        ctx.set_phase_stamps(False)


def same_bytes(a, b, label):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, tuple):
            same_bytes(x, y, f"{label}[{k}]")
        else:
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{label}: output {k} differs between the production and the diagnostic build"


# ---- 1. results ----------------------------------------------------------------------------------------------------------
SE_CASES = [("rep", "records", 0, 100), ("rep", "records", 2, 150), ("rep", "planes", 1, 100), ("rep", "planes", 2, 240),
            ("unique", "records", 1, 100), ("unique", "planes", 0, 100), ("iupac", "nibbles", 0, 100), ("iupac", "nibbles", 2, 100)]


def filter_ctx(bed, flt):
    """the context whose batches of up to 172 bases run the named filter form, its path asserted"""
    # (a genome with IUPAC letters has no bit planes and gets no seed-extension tables)
    ctx = bed.ctx(letters=(0, 0) if flt == "nibbles" else (2, 1), records=172 if flt == "records" else 0, direct=None)
    assert ctx.filter_on_planes() == (flt != "nibbles")
    assert ctx.window_records() == (172 if flt == "records" else 0)
    return ctx


@pytest.mark.parametrize("bed_name,flt,mode,L", SE_CASES, ids=[f"{b}-{f}-m{m}-L{L}" for b, f, m, L in SE_CASES])
def test_se_results(beds, bed_name, flt, mode, L):
    bed = beds(bed_name)
    ctx = filter_ctx(bed, flt)
    reads = bed.reads(mode, L)
    o_res, o_cig, o_n, _ = bed.expected_se(reads, mode, ("se", mode, L))
    plain = ctx.map_se(reads, mode=mode)
    assert all(v == 0 for v in ctx.take_work().values()), "the production build kept a tally"
    diag, tiers = stamped(ctx, lambda: ctx.map_se(reads, mode=mode))
    same_bytes(plain, diag, f"SE {bed_name} {flt} mode {mode} L {L}")
    compare_se(*diag, o_res, o_cig, o_n, reads, f"SE diagnostic build, {bed_name} {flt} mode {mode} L {L}")
    t = tiers[0]
    assert t["cyc_total"] > 0 and t["seed_offsets"] > 0 and t["candidates"] > 0, t
    assert all(v == 0 for v in tiers[1].values()), "single-end launches tally into the first 16 words"
    if flt == "records":
        assert t["window_cache_hits"] == 0, "the record-fed build has no position cache"
    elif bed_name != "unique":
        assert 0 < t["window_cache_hits"] <= t["candidates"]
    assert (diag[0]["pos"] != 0).mean() > 0.5


PE_CASES = [("rep", "planes", "unsplit", 0), ("rep", "planes", "split", 1), ("rep", "planes", "split_stage_16384", 2),
            ("rep", "records", "unsplit", 2), ("rep", "records", "split", 0), ("rep", "records", "split_stage_16384", 1),
            ("iupac", "nibbles", "unsplit", 1), ("iupac", "nibbles", "split", 2), ("iupac", "nibbles", "split_stage_16384", 0),
            ("unique", "records", "split", 0)]


@pytest.mark.parametrize("bed_name,flt,form,mode", PE_CASES, ids=[f"{b}-{f}-{fo}-m{m}" for b, f, fo, m in PE_CASES])
def test_pe_results(beds, bed_name, flt, form, mode):
    bed = beds(bed_name)
    ctx = filter_ctx(bed, flt)
    r1, r2 = bed.pairs(mode)
    n = len(r1)
    orc = bed.expected_pe(r1, r2, mode, ("pe", mode))
    ctx.set_pe_split(**FORM[form])
    plain = ctx.map_pe(r1, r2, mode=mode)
    prod = ctx.take_work_tiers()
    ctx.pe_split_stats()
    diag, tiers = stamped(ctx, lambda: ctx.map_pe(r1, r2, mode=mode))
    st = ctx.pe_split_stats()
    label = f"PE {bed_name} {flt} {form} mode {mode}"
    print(label, "routes", st, "tier 1", tiers[0], "tier 2", tiers[1])
    same_bytes(plain, diag, label)
    compare_pe(diag, orc, label + ", diagnostic build")
    t1, t2 = tiers
    assert t1["cyc_total"] > 0 and t1["seed_offsets"] > 0 and t1["candidates"] > 0 and t1["alignments"] > 0, t1
    routed = st["mated_from_lds"] + st["mapped_whole"] + st["mated_from_device_memory"]
    if form == "unsplit":
        assert routed == 0, st
    else:
        assert routed == n and st["mated_from_lds"] > 0, st
    if bed_name == "unique":
        assert idle(t2) and st["mapped_whole"] == st["mated_from_device_memory"] == 0, (t2, st)
    else:
        # the bed is there to make tier 2 run: the whole-pair kernel (the only one that seeds in tier 2) and, with a staging
        # area, the mate kernel on lists in device memory
        assert t2["cyc_total"] > 0 and t2["seed_offsets"] > 0 and t2["alignments"] > 0, t2
        if form == "split":
            assert st["mapped_whole"] > 0 and st["mated_from_device_memory"] == 0, st
        if form == "split_stage_16384":
            assert st["mated_from_device_memory"] > 0, st
    # the production builds: no seed-pass count and no cycles in either tier; what they do keep is pinned in
    # test_production_builds_keep_no_seed_tallies
    for t in prod:
        assert all(t[k] == 0 for k in ("seed_offsets", "search_probes", "candidates", "index_run_lines", "window_cache_hits", "cyc_total")), prod


def sliced_with_tails(ctx, reads, mode, bam):
    ctx.set_sam_tails(True)
    ctx.set_record_format(bam=bam)
    try:
        return ctx.map_se_sliced(reads, [0, 300, 1100, len(reads)], mode=mode, tails=True)
    finally:
        ctx.set_sam_tails(False)
        ctx.set_record_format(bam=False)


@pytest.mark.parametrize("flt", ["records", "planes"])
def test_se_sliced_and_sam_text_under_the_stamps(beds, flt):
    """abm_map_se_batch_sliced through the diagnostic build, without and with SAM tails: results and text are the production
    build's; with BAM pieces asked for the diagnostic build writes none (se_text_stride: every read is left to the host)
    and the results are unchanged"""
    bed = beds("unique")
    ctx = filter_ctx(bed, flt)
    reads = bed.reads(2)
    o_res, o_cig, o_n, _ = bed.expected_se(reads, 2, ("se", 2, 100))
    cuts = [0, 300, 1100, len(reads)]
    plain = ctx.map_se_sliced(reads, cuts, mode=2)[:3]
    diag, tiers = stamped(ctx, lambda: ctx.map_se_sliced(reads, cuts, mode=2)[:3])
    same_bytes(plain, diag, "sliced")
    compare_se(*diag, o_res, o_cig, o_n, reads, "sliced, diagnostic build")
    assert tiers[0]["cyc_total"] > 0
    text_p = sliced_with_tails(ctx, reads, 2, bam=False)
    text_d, tiers = stamped(ctx, lambda: sliced_with_tails(ctx, reads, 2, bam=False))
    assert tiers[0]["cyc_total"] > 0
    same_bytes(plain, text_d[:3], "sliced with SAM tails")
    assert text_p[4] == text_d[4], "SAM text differs between the production and the diagnostic build"
    written = [t for t in text_d[4] if t]
    # (the rest: unmapped reads, and CIGARs beyond the 4-op slot, which are the host's to format)
    assert len(written) > 0.5 * sum(1 for r in reads if r) and all(t.endswith(b"\n") for t in written)
    bam_p = sliced_with_tails(ctx, reads, 2, bam=True)
    assert sum(1 for t in bam_p[4] if t) == len(written), "the production build writes BAM pieces"
    bam_d, tiers = stamped(ctx, lambda: sliced_with_tails(ctx, reads, 2, bam=True))
    assert tiers[0]["cyc_total"] > 0
    same_bytes(plain, bam_d[:3], "sliced, BAM pieces asked of the diagnostic build")
    assert all(t is None for t in bam_d[4]), "the diagnostic build has no BAM form: every record is the host's"


def test_pe_text_is_refused_under_the_stamps(beds):
    """paired SAM text (and BAM pieces) with the stamps on: pe_text_stride answers 0, the batch has no text and the results
    are those of a run without text"""
    bed = beds("unique")
    ctx = filter_ctx(bed, "planes")
    r1, r2 = bed.pairs(0)
    plain = ctx.map_pe(r1, r2, mode=0)
    for bam in (False, True):
        ctx.set_sam_tails(True)
        ctx.set_record_format(bam=bam)
        try:
            prod = ctx.map_pe(r1, r2, mode=0, sam=True)
            diag, tiers = stamped(ctx, lambda: ctx.map_pe(r1, r2, mode=0, sam=True))
        finally:
            ctx.set_sam_tails(False)
            ctx.set_record_format(bam=False)
        assert prod[5] is not None and (prod[5] == 0).sum() > 0, "the production build writes the text"
        assert diag[5] is None and diag[6] is None
        same_bytes(plain, prod[:5], "production, text")
        same_bytes(plain, diag[:5], "diagnostic, text asked for")
        assert tiers[0]["cyc_total"] > 0


# ---- 2. tallies ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bed_name", ["unique", "rep"])
def test_se_seed_tallies_equal_the_oracle(beds, bed_name):
    """Plain configuration (no tables, no direct narrowing, no records), mode 2 (four orientation calls a read).

    The kernel and the oracle walk the same offsets (n_off of seed_pass = spec_lim / n_off of seed_passes), look at the
    same buckets (chk2 / chk3 = the two scan_bucket conditions) and apply the same candidates in the same order (replay).
    They differ in WHEN they stop once
    the set is sure_ambig (two different exact matches): the oracle leaves its loops at that candidate, the kernel has
    counted its whole block of 64 offsets (and narrowed all of them) and counts the whole step of 128 candidates.
    sure_ambig is sticky for the rest of the read, and a read that was sure_ambig comes out with flag 0x100 (choose_se
    returns the exact match as it stands).  Hence, with the batch split by the oracle's own flag and each part mapped alone:

      reads without 0x100 (unmapped ones included)   EXACT: seed_offsets == seed_iters, candidates == candidates,
                                                     set_updates == set_updates; search_probes: see below
      reads with 0x100, n of them                    TWO-SIDED: oracle <= kernel <= oracle + 63 n (offsets: the rest of one
                                                     block, once per read), <= oracle + 127 n (candidates: the rest of one
                                                     step), and set_updates likewise within 127 n (an update is a candidate
                                                     of that step); search_probes >= the oracle's unshared ones, no upper
                                                     bound (the block's other offsets are narrowed too): printed.

    search_probes -- NOT equal, as one might expect from narrow_both replaying first_not's halving (it does: the boundaries
    are std::lower_bound's, tests/hip/narrow_check.hip).  The oracle counts every probe of every bisection: one bisection per
    letter on the 2-letter table, two (first symbol >= mid, first symbol >= top) on a 3-letter table.  narrow_both runs the
    two 3-letter bisections of a letter in lockstep and counts a round in which both probe the SAME entry once
    (`d2 = ... && !(d1 && m2 == m1)`: one load serves both) -- they start at the same midpoint, so that is at least the first
    round of every letter.  The k-th round of a letter is the k-th probe of each bisection, so the oracle can say how many
    probes were shared: `shared_probes3` (the entries first_not probed, compared round by round).  EXACT for the unflagged
    reads:  search_probes == oracle search_probes - shared_probes3, with shared_probes3 > 0 on the rep bed.  (Observed on
    rep, 1498 unflagged reads of 100 bases, mode 2: kernel 1,938,790, oracle 3,644,345.)

    alignments: choose_se / choose_se_pilot count one per job of the read's set (a lone job once, else every `select`),
    the oracle's `aligns` one scoring run per job and `aligns_tb` the winner's traceback: EXACT alignments == aligns, so
    alignments <= aligns + aligns_tb; a mapped read whose hit is not an exact match (exact matches are never aligned) had
    at least one job, so alignments >= their number."""
    bed = beds(bed_name)
    ctx = bed.ctx()
    reads = bed.reads(2)
    o_res, o_cig, o_n, _ = bed.expected_se(reads, 2, ("se", 2, 100))
    flagged = (o_res["flags"] & 0x100) != 0
    clear = [r for r, f in zip(reads, flagged) if not f]
    ambig = [r for r, f in zip(reads, flagged) if f]
    oc = bed.oracle.map_se(bed.oix, clear, mode=2, threads=8)
    w = se_tally(ctx, clear, 2)
    print(bed_name, "reads the oracle does not flag:", len(clear), "kernel", w, "oracle", oc[3])
    assert w["seed_offsets"] == oc[3]["seed_iters"] > 0
    assert w["candidates"] == oc[3]["candidates"] > 0
    assert w["set_updates"] == oc[3]["set_updates"] > 0
    assert w["search_probes"] == oc[3]["search_probes"] - oc[3]["shared_probes3"]
    if bed_name == "rep":
        assert w["search_probes"] > 0 and oc[3]["shared_probes3"] > 0, "the bed no longer narrows 3-letter ranges"
    assert w["alignments"] == oc[3]["aligns"] <= oc[3]["aligns"] + oc[3]["aligns_tb"]
    exact = np.array([int(oc[0][i]["diffs"]) == 0 and int(oc[2][i]) == 1 for i in range(len(clear))], dtype=bool)
    assert w["alignments"] >= int(((oc[0]["pos"] != 0) & ~exact).sum()) > 0
    assert w["phase_cycles"]["align"] > 0
    if bed_name == "rep":
        assert len(ambig) > 20, "the bed no longer has reads with two exact matches"
    if not ambig:
        return
    oa = bed.oracle.map_se(bed.oix, ambig, mode=2, threads=8)[3]
    wa = se_tally(ctx, ambig, 2)
    n = len(ambig)
    print(bed_name, "reads the oracle flags ambiguous:", n, "kernel", wa, "oracle", oa)
    assert oa["seed_iters"] <= wa["seed_offsets"] <= oa["seed_iters"] + 63 * n
    assert oa["candidates"] <= wa["candidates"] <= oa["candidates"] + 127 * n
    assert oa["set_updates"] <= wa["set_updates"] <= oa["set_updates"] + 127 * n
    assert wa["search_probes"] >= oa["search_probes"] - oa["shared_probes3"]
    assert wa["alignments"] == oa["aligns"]


def test_se_tallies_across_index_configurations(beds):
    """Seed-extension tables, direct narrowing and window records change how a bucket is found and where a window is read
    from, never which offsets are walked, which buckets are checked or what enters the set: seed_offsets, candidates and
    set_updates are EXACTLY those of the plain configuration, for the whole batch (reads with two exact matches included: the
    kernel's stopping place is a function of the candidates' order alone).  The tables answer for most offsets with one
    load in the place of bisections: 0 < probes < plain's, strictly (tables that tabulate nothing would give equality; what the
    tables hold is compared key by key in tests/test_gpu_index_derived.py).  With direct narrowing the count is whatever narrow_direct's
    own search takes: printed, non-zero."""
    bed = beds("rep")
    reads = bed.reads(0)
    configs = {"plain": dict(), "tables": dict(letters=(3, 2)), "direct": dict(direct=None), "records": dict(records=108),
               "all": dict(letters=(3, 2), records=108, direct=None)}
    got = {name: se_tally(bed.ctx(**kw), reads, 0) for name, kw in configs.items()}
    for name, w in got.items():
        print(f"rep, 2000 reads of 100 bases, mode 0, {name}: search_probes {w['search_probes']}", {k: w[k] for k in SEED_KEYS})
        for k in ("seed_offsets", "candidates", "set_updates", "alignments"):
            assert w[k] == got["plain"][k] > 0, (name, k)
        assert w["search_probes"] > 0
    assert got["tables"]["search_probes"] < got["plain"]["search_probes"]
    assert got["records"]["search_probes"] == got["plain"]["search_probes"], "the single-end kernel bisects on the nibble array with records too"
    assert got["records"]["window_cache_hits"] == got["all"]["window_cache_hits"] == 0
    assert 0 < got["plain"]["window_cache_hits"] <= got["plain"]["candidates"]


def words_per_window(L, planes, records):
    """abismal_amd.h / seed_pass: 8-byte words fetched per candidate window.  On the bit planes G lanes share a window
    (single-end: 2 up to 128 bases, 4 up to 192, 8 up to 448, beyond that the nibble array): a pair of lanes fetches 6
    words, a group of four 8, a group of eight two per 64-base block the window can touch; a record is read as 6 words by two
    lanes and 8 by four; on the nibble array a lane reads the read's own ceil(L / 16) words"""
    if not planes or L > 448:
        return (L + 15) // 16
    g = 2 if L <= 128 else (4 if L <= 192 else 8)
    if records:
        assert g in (2, 4)
        return 6 if g == 2 else 8
    return 6 if g == 2 else (8 if g == 4 else 2 * ((L + 63) // 64 + 1))


@pytest.mark.parametrize("L", [100, 150, 240, 460])
def test_read_words_per_window(beds, L):
    """EXACT: read_words == candidates x words_per_window(L) on batches of one length (the figure is a function of the read's
    length), on the planes, on records where they serve (100: two lanes; 150: four) and on the nibble array of a genome
    with IUPAC letters; 460 bases is beyond the planes' reach (the nibble build on a genome that has planes)"""
    rep, iupac = beds("rep"), beds("iupac")
    cases = [(rep, rep.ctx(), True, False), (iupac, iupac.ctx(), False, False)]
    if L <= 172:
        cases.append((rep, rep.ctx(records=172), True, True))
    for bed, ctx, planes, records in cases:
        reads = bed.reads(0, L, n=600, uniform=True)
        assert len(reads) > 400 and ctx.filter_on_planes() == planes
        w = se_tally(ctx, reads, 0)
        per = words_per_window(L, planes, records)
        print(f"L {L} {bed.name} records {records}: candidates {w['candidates']}, read_words {w['read_words']}, {per} per window")
        assert w["candidates"] > 0 and w["read_words"] == w["candidates"] * per
        assert (w["window_cache_hits"] == 0) if records else (0 < w["window_cache_hits"] <= w["candidates"])


def shuffled_mates(r1, r2):
    """every fourth pair gets another pair's second end: its ends map, if at all, on their own (fallback hits)"""
    r2 = list(r2)
    for k in range(0, len(r2) - 4, 4):
        r2[k] = r2[k + 2]
    return r1, r2


def lines_bounds(t, complete):
    """index_run_lines (the oracle does not expose its checked buckets, so a TWO-SIDED bound): a checked bucket of n >= 1
    entries starting at entry lo spans ((lo + n - 1) >> 5) - (lo >> 5) + 1 lines of 32 entries -- at least n / 32, less than
    n / 32 + 2 -- and an offset checks at most two buckets, whose n add up to `candidates`:
        candidates / 32 <= lines <= candidates / 32 + 4 seed_offsets.
    complete = no seed pass stopped inside a block (the lines of a block are counted before its candidates are taken, so a
    block left early has lines without candidates: there only the lower bound holds)"""
    assert 32 * t["index_run_lines"] >= t["candidates"] > 0, t
    if complete:
        assert 32 * t["index_run_lines"] <= t["candidates"] + 128 * t["seed_offsets"], t


def idle(tier):
    """a tier no pair reached: every word zero but cyc_total -- the launch still starts its waves, each of which adds the
    cycles between its first and its last stamp"""
    return all(v == 0 for k, v in tier.items() if k != "cyc_total")


@pytest.mark.parametrize("mode", [0, 2])
def test_pe_tallies_on_unique_equal_the_oracle(beds, mode):
    """Plain configuration.  On a genome without repeats no set outgrows tier 1 (256 entries) and none is ever sure_ambig
    (PeSet: a FULL set whose cutoff is 0 -- 32 exact matches or more), so nothing stops early: tier 1's seed_offsets,
    candidates EXACTLY equal the oracle's, search_probes the oracle's minus shared_probes3 (see
    test_se_seed_tallies_equal_the_oracle, which is where that relation is put to the test: a genome without repeats has
    no bucket of two entries, so both sides are 0 here at any -c; the pair kernels narrow with the same narrow_both), and
    so do its set_updates -- seed_pass counts what enters the
    pair sets (append / admit = scan_bucket's admits), feed_single what best_single feeds the single-end sets (the
    oracle's second `++work.set_updates`, in orientation()).  The same for every launch form: unsplit (one kernel counts
    all), split (the seed kernel counts the seed passes, the mate kernel the best_single updates), split with a staging
    area.  Tier 2: no pair routed to it and every word zero but cyc_total (idle(): its launches still start waves).  alignments: >= one per end of a mated pair (score_pairable),
    printed beside the oracle's aligns (the kernel scores pairable entries only, the oracle memoises: no equality)."""
    bed = beds("unique")
    ctx = bed.ctx()
    r1, r2 = shuffled_mates(*bed.pairs(mode))
    orc = bed.expected_pe(r1, r2, mode, ("pe-shuffled", mode))
    ow = orc[5]
    assert (orc[1]["pos"] != 0).sum() > 50, "the batch is built to have fallback hits"
    for form in PE_FORMS:
        ctx.set_pe_split(**FORM[form])
        gpu, (t1, t2) = stamped(ctx, lambda: ctx.map_pe(r1, r2, mode=mode))
        st = ctx.pe_split_stats()
        print(f"unique PE mode {mode} {form}: tier 1", t1, "oracle", ow, "routes", st)
        compare_pe(gpu, orc, f"unique PE mode {mode} {form}")
        assert idle(t2), t2
        assert st["mapped_whole"] == st["mated_from_device_memory"] == 0
        assert st["mated_from_lds"] == (0 if form == "unsplit" else len(r1))
        assert t1["seed_offsets"] == ow["seed_iters"] > 0
        assert t1["candidates"] == ow["candidates"] > 0
        assert t1["search_probes"] == ow["search_probes"] - ow["shared_probes3"]
        assert t1["set_updates"] == ow["set_updates"] > 0
        lines_bounds(t1, complete=True)
        mated = int((orc[0]["r1"]["pos"] != 0).sum())
        assert t1["alignments"] >= 2 * mated > 0
        # cycle stamps: the eight parts lie inside the total, and a phase that did work shows it
        assert sum(t1[k] for k in PE_CYCLE_PARTS) <= t1["cyc_total"]
        assert all(t1[k] > 0 for k in PE_CYCLE_PARTS), t1  # (cyc_se_fallback: the shuffled mates)


def test_pe_tallies_on_rep_by_tier(beds):
    """Repeat-rich genome, plain configuration, every launch form.  Tier 1 does, for each pair, a PREFIX of the oracle's
    work (identical until a set outgrows 256 entries -- or the seed kernel's staging area, or the hand-over area -- and
    the pair is abandoned to tier 2) or all of it; tier 2 (the whole-pair kernel) does ALL of the oracle's work for the
    pairs it redoes; either may run on to the end of its block of 64 offsets / step of 128 candidates where the oracle
    stops at once (sure_ambig; tier 1 also where it abandons).  Per seed_pass call that is at most 63 offsets and 127
    candidates, and a pair has at most 16 calls per tier (2 ends x 4 orientation calls x 2 passes).  TWO-SIDED, for
    seed_offsets and candidates:   oracle <= tier 1 + tier 2,   each tier <= oracle + 16 x n x (63 | 127).
    (The unsplit / split equality on the unique bed is the exact check; this one shows that tier 2 is counted once and
    apart.)  take_work() == tier 1 + tier 2 element by element (the counts; cycles differ from run to run);
    index_run_lines within lines_bounds."""
    bed = beds("rep")
    ctx = bed.ctx()
    r1, r2 = bed.pairs(0)
    n = len(r1)
    orc = bed.expected_pe(r1, r2, 0, ("pe", 0))
    ow = orc[5]
    for form in PE_FORMS:
        ctx.set_pe_split(**FORM[form])
        _, (t1, t2) = stamped(ctx, lambda: ctx.map_pe(r1, r2, mode=0))
        st = ctx.pe_split_stats()
        print(f"rep PE {form}: tier 1", t1, "tier 2", t2, "oracle", ow, "routes", st)
        assert t2["seed_offsets"] > 0 and t2["candidates"] > 0 and t2["alignments"] > 0 and t2["cyc_total"] > 0
        for mine, theirs, slack in (("seed_offsets", "seed_iters", 63), ("candidates", "candidates", 127)):
            assert ow[theirs] <= t1[mine] + t2[mine], (form, mine)
            assert t1[mine] <= ow[theirs] + 16 * n * slack and t2[mine] <= ow[theirs] + 16 * n * slack, (form, mine)
        for t in (t1, t2):
            lines_bounds(t, complete=False)
            assert sum(t[k] for k in PE_CYCLE_PARTS) <= t["cyc_total"]
        if form != "unsplit":
            continue
        # (either call resets the tallies, so the sum is taken from a second run -- of the one form whose routes do not
        # depend on the order waves finish in: in the split forms the hand-over area of a repeat-rich batch runs out, and
        # which pairs find no room there and are mapped whole differs from run to run)
        ctx.take_work()
        ctx.set_phase_stamps(True)
        try:
            ctx.map_pe(r1, r2, mode=0)
            total = ctx.take_work()
        finally:
            ctx.set_phase_stamps(False)
        both = {k: t1[k] + t2[k] for k in COUNT_KEYS}
        assert {k: total["read_words" if k == "index_run_lines" else k] for k in COUNT_KEYS} == both


def test_tallies_add_up_and_reset(beds):
    """a second take_work() returns zeros; tallies of A plus tallies of B are those of A then B with no take in between; a
    batch mapped in one call and in four quarters tallies the same (neither grid size nor the order reads are taken in
    matters) -- single-end and paired"""
    bed = beds("unique")
    ctx = bed.ctx()
    reads = bed.reads(2)
    keys = ("seed_offsets", "search_probes", "candidates", "read_words", "set_updates", "alignments", "window_cache_hits")
    whole = se_tally(ctx, reads, 2)
    again = ctx.take_work()
    assert all(v == 0 for v in again.values()) and "phase_cycles" not in again, again
    assert all(v == 0 for t in ctx.take_work_tiers() for v in t.values())
    half = len(reads) // 2
    a, b = se_tally(ctx, reads[:half], 2), se_tally(ctx, reads[half:], 2)
    ctx.set_phase_stamps(True)
    try:
        ctx.map_se(reads[:half], mode=2)
        ctx.map_se(reads[half:], mode=2)
        ab = ctx.take_work()
        q = len(reads) // 4
        for k in range(4):
            ctx.map_se(reads[k * q:(k + 1) * q if k < 3 else len(reads)], mode=2)
        quarters = ctx.take_work()
        r1, r2 = bed.pairs(0)
        ctx.map_pe(r1, r2, mode=0)
        pe_whole = ctx.take_work_tiers()
        assert all(v == 0 for t in ctx.take_work_tiers() for v in t.values())
        hp = len(r1) // 2
        ctx.map_pe(r1[:hp], r2[:hp], mode=0)
        ctx.map_pe(r1[hp:], r2[hp:], mode=0)
        pe_halves = ctx.take_work_tiers()
        ctx.map_pe(r1, r2, mode=0)
        pe_sum = ctx.take_work()  # (the header's promise: take_work returns the tiers' sum)
    finally:
        ctx.set_phase_stamps(False)
    for k in keys:
        assert a[k] + b[k] == ab[k] == whole[k] == quarters[k], k
    assert whole["seed_offsets"] > 0 and whole["alignments"] > 0
    for k in COUNT_KEYS:
        assert pe_whole[0][k] == pe_halves[0][k] and pe_whole[1][k] == pe_halves[1][k] == 0, k
        assert pe_sum["read_words" if k == "index_run_lines" else k] == pe_whole[0][k] + pe_whole[1][k], k
    assert pe_whole[0]["seed_offsets"] > 0


def test_production_builds_keep_no_seed_tallies(beds):
    """What take_work / take_work_tiers return with the stamps off, as include/abismal_amd.h states it: the single-end
    kernel keeps nothing at all; the pair kernels keep no seed-pass count ([0]-[3], [11]) and no cycles, only what costs
    them nothing: [4] the best_single updates (feed_single counts unconditionally) -- fewer than the diagnostic builds' [4],
    which adds the seed passes' -- and [5] the alignments, equal to the diagnostic builds': tier by tier when one kernel
    maps a pair, in sum over the tiers in the split forms (there a pair whose lists find no room in the hand-over area is
    mapped whole in tier 2, and which pairs those are depends on the order the seed kernel's waves finish in)."""
    bed = beds("rep")
    ctx = bed.ctx()
    ctx.map_se(bed.reads(0), mode=0)
    w = ctx.take_work()
    assert all(v == 0 for v in w.values()) and "phase_cycles" not in w, w
    r1, r2 = bed.pairs(0)
    for form in ("unsplit", "split"):
        ctx.set_pe_split(**FORM[form])
        ctx.take_work()
        ctx.map_pe(r1, r2, mode=0)
        prod = ctx.take_work_tiers()
        _, diag = stamped(ctx, lambda: ctx.map_pe(r1, r2, mode=0))
        ctx.pe_split_stats()
        print(f"rep PE {form}: production", prod, "diagnostic", diag)
        for p, d in zip(prod, diag):
            assert all(v == 0 for k, v in p.items() if k not in ("set_updates", "alignments")), p
            assert p["alignments"] > 0 and (form != "unsplit" or p["alignments"] == d["alignments"])
        assert prod[0]["alignments"] + prod[1]["alignments"] == diag[0]["alignments"] + diag[1]["alignments"]
        assert 0 < prod[0]["set_updates"] + prod[1]["set_updates"] < diag[0]["set_updates"] + diag[1]["set_updates"]
        ctx.map_pe(r1, r2, mode=0)
        total = ctx.take_work()
        if form == "unsplit":
            assert total["set_updates"] == prod[0]["set_updates"] + prod[1]["set_updates"]
        assert total["alignments"] == prod[0]["alignments"] + prod[1]["alignments"]
        assert total["seed_offsets"] == total["candidates"] == total["read_words"] == 0 and "phase_cycles" not in total


# ---- 3. cycle stamps ---------------------------------------------------------------------------------------------------------
CANARY = -0x12345679


def test_se_cycles_and_the_per_read_array(beds):
    import torch
    bed = beds("rep")
    ctx = bed.ctx(letters=(2, 1), records=172, direct=None)
    reads = bed.reads(2)
    n = len(reads)
    w = se_tally(ctx, reads, 2)
    pc = w["phase_cycles"]
    assert all(v >= 0 for v in pc.values())
    assert pc["probe_narrow"] + pc["gather_hamming"] + pc["replay"] + pc["align"] <= pc["total"]
    assert w["alignments"] > 0 and all(pc[k] > 0 for k in ("probe_narrow", "gather_hamming", "replay", "align")), pc
    cyc = torch.full((n + 64,), CANARY, dtype=torch.int32, device="cuda")
    ctx.set_read_cycles(cyc.data_ptr())
    try:
        ctx.map_se(reads, mode=2)  # stamps off: the production build never sees the array
        torch.cuda.synchronize()
        assert bool((cyc == CANARY).all())
        stamped(ctx, lambda: ctx.map_se(reads, mode=2))
        torch.cuda.synchronize()
        got = cyc.cpu().numpy()
    finally:
        ctx.set_read_cycles(None)
    assert (got[:n] != CANARY).all(), "a read's entry was not written"
    assert (got[:n] >= 0).all() and got[:n].max() > 0
    assert (got[n:] == CANARY).all(), "written beyond the batch"
    cyc.fill_(CANARY)
    stamped(ctx, lambda: ctx.map_se(reads, mode=2))  # (array taken away: the diagnostic build writes nowhere)
    torch.cuda.synchronize()
    assert bool((cyc == CANARY).all())


@pytest.mark.parametrize("bed_name,form", [("unique", "split"), ("unique", "unsplit"), ("rep", "split_stage_16384"), ("rep", "unsplit")])
def test_pe_per_pair_arrays(beds, bed_name, form):
    """set_read_cycles for pairs: largest set << 16 | cycles >> 20, one word per pair, by whichever kernel finished the
    pair; set_pair_phases: [n][8], added to"""
    import torch
    bed = beds(bed_name)
    ctx = bed.ctx(letters=(2, 1), records=172, direct=None)
    r1, r2 = bed.pairs(0)
    n = len(r1)
    orc = bed.expected_pe(r1, r2, 0, ("pe", 0))
    ctx.set_pe_split(**FORM[form])
    diag = torch.full((n + 64,), CANARY, dtype=torch.int32, device="cuda")
    phases = torch.zeros((n + 8, 8), dtype=torch.int32, device="cuda")
    ctx.set_read_cycles(diag.data_ptr())
    ctx.set_pair_phases(phases.data_ptr())
    try:
        ctx.map_pe(r1, r2, mode=0)  # stamps off
        torch.cuda.synchronize()
        assert bool((diag == CANARY).all()) and not bool(phases.any())
        _, (t1, t2) = stamped(ctx, lambda: ctx.map_pe(r1, r2, mode=0))
        torch.cuda.synchronize()
        words = diag.cpu().numpy().copy()
        first = phases.cpu().numpy().copy()
        stamped(ctx, lambda: ctx.map_pe(r1, r2, mode=0))
        torch.cuda.synchronize()
        second = phases.cpu().numpy().copy()
        ctx.set_pair_phases(None)
        stamped(ctx, lambda: ctx.map_pe(r1, r2, mode=0))
        torch.cuda.synchronize()
        third = phases.cpu().numpy().copy()
    finally:
        ctx.set_read_cycles(None)
        ctx.set_pair_phases(None)
    assert (words[:n] != CANARY).all() and (words[n:] == CANARY).all()
    sets = words[:n].view(np.uint32) >> 16
    found = (orc[0]["r1"]["pos"] != 0) | (orc[1]["pos"] != 0) | (orc[2]["pos"] != 0)
    assert found.sum() > 0.5 * n and (sets[found] >= 1).all()
    tier2_ran = not idle(t2)
    print(f"{bed_name} {form}: largest set {sets.max()}, pairs beyond {TIER1_CAP}: {(sets > TIER1_CAP).sum()}, tier 2 ran: {tier2_ran}")
    assert bool((sets > TIER1_CAP).any()) == tier2_ran == (bed_name == "rep")
    assert not first[n:].any() and not second[n:].any(), "written beyond the batch"
    mated = orc[0]["r1"]["pos"] != 0
    assert mated.sum() > 0.3 * n and first[:n][mated].any(axis=1).all(), "a mated pair's row is empty"
    assert (first >= 0).all() and (second >= first).all() and (second[:n][mated].sum(axis=1) > first[:n][mated].sum(axis=1)).all()
    assert (third == second).all(), "set_pair_phases(NULL) did not stop the writes"


# ---- 4. launch timers ------------------------------------------------------------------------------------------------------
def test_launch_timers(beds):
    """abm_ctx_set_timing: one bracket per single-end batch -- the batch's main launch; the launches se_long_reads adds for
    reads beyond 1024 bases (the is_long build, one launch per 1024 such reads) are NOT inside timed_launch, so a batch with such a
    read still records one, as abismal_amd.h says -- and pe_timed_launches() per paired batch: 2 unsplit (tier 1, tier 2),
    4 split (seed, mate, mate on lists in device memory, whole pairs)"""
    import torch
    bed = beds("unique")
    ctx = bed.ctx(letters=(2, 1), records=172, direct=None)
    reads = bed.reads(0)
    r1, r2 = bed.pairs(0)
    chrom = synth.read_chroms(bed.fa)[0]
    long_read = bytes(chrom[5000:5000 + LDS_READ_LEN + 200]).decode().replace("C", "T")
    ctx.map_se(reads, mode=0)  # (workspaces grown, occupancy queried: outside the timed calls)
    ctx.map_se(reads[:50] + [long_read], mode=0)
    for form in ("unsplit", "split"):
        ctx.set_pe_split(**FORM[form])
        ctx.map_pe(r1, r2, mode=0)
    assert ctx.take_kernel_times() == [], "launches were timed before set_timing"
    ctx.set_timing(True)
    try:
        k = 3
        t0 = time.perf_counter()
        for _ in range(k):
            ctx.map_se(reads, mode=0)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ms = ctx.take_kernel_times()
        print(f"{k} single-end calls: {ms} ms in {wall:.2f} ms of wall time")
        assert len(ms) == k and all(x > 0 for x in ms) and sum(ms) <= wall
        assert ctx.take_kernel_times() == [] and ctx.take_kernel_time() == (0, 0.0)
        res = ctx.map_se(reads[:50] + [long_read], mode=0)[0]
        assert int(res[50]["pos"]) != 0, "the long read was not mapped"
        assert len(ctx.take_kernel_times()) == 1
        for form, per_call in (("unsplit", 2), ("split", 4)):
            ctx.set_pe_split(**FORM[form])
            t0 = time.perf_counter()
            for _ in range(k):
                ctx.map_pe(r1, r2, mode=0)
                assert ctx.pe_timed_launches() == per_call
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            ms = ctx.take_kernel_times()
            print(f"{k} paired calls, {form}: {ms} ms in {wall:.2f} ms of wall time")
            assert len(ms) == k * per_call and all(x > 0 for x in ms) and sum(ms) <= wall
        ctx.map_se(reads, mode=0)
        n, total = ctx.take_kernel_time()
        assert n == 1 and total > 0 and ctx.take_kernel_time() == (0, 0.0)
    finally:
        ctx.set_timing(False)
    ctx.map_se(reads, mode=0)
    ctx.map_pe(r1, r2, mode=0)
    assert ctx.take_kernel_times() == [] and ctx.take_kernel_time() == (0, 0.0)
