"""GPU parity where paired-end candidate sets reach their limit of kPeCapLarge = 32768 entries: everything downstream of
PeSet in the whole-pair kernel ("tier 2") -- the radix sort of sort_unique on lists of tens of thousands of entries, the
sampled binary search at samp_shift up to 6, freeze_heap_order / heap_order_now on a full heap, the best-single log and
replay_singles, a set that is full and evicting, worth == false (a full set at cutoff 0: the mating is skipped) and mating
windows wider than one 64-step chunk -- against the oracle, bit for bit (pair, both fallback hits, both CIGARs:
compare_pe / compare_se; no tolerances).

The fixture (tests/synth.py: satellite_genome, pairs_on_satellite, reads_on_satellite): one random unit of 200 bases
planted COPIES = 30000 times, evenly spaced, all on one strand, and pairs of 2 x 100 cut from the copies, fully converted,
mapped with max_candidates = 30000 so that no bucket is narrowed and an end finds every copy.  Three genomes:

  near        2.5 % divergence between the copies.  Tuned on the oracle: at 1 % and 2 % too many pairs are ambiguous (an
              end whose copy carries no substitution has thousands of equals: 35 of 64 at 2 %, 19 unique), at 3 % no set
              fills any more (measured with 24000 copies), at 2.5 % sets fill and evict -- 35 of the 64 pairs fill one,
              289446 admissions into a full set -- and the oracle reports, of 64 pairs (default limits / max_frag 40000 /
              150-300): 28 / 22 / 42 unique, 26 / 36 / 11 ambiguous, 10 / 6 / 11 with fallback hits only.
  exact       0 %, and pairs without planted differences: every set is full at cutoff 0 (sure_ambig stops the seed
              passes) and the mating is skipped, so no list is ever sorted and, in mode 0, nothing is aligned: 64 of 64
              pairs are reported end by end.  Its floors are alive_exact's, not alive_near's.
  near_iupac  `near` with 400 ambiguity letters in the flanks: no bit planes, the filter stays on the nibble array.

Half of the pairs carry 1-3 planted substitutions per end, a quarter of those a one-base indel per end as well (winners
decided by the DP, gapped tracebacks), and one pair in eight has its second end on the same strand as the first: its ends
find the family in different orientation calls, so it is reported end by end from full sets (replay_singles).

Every test first asserts, on the ORACLE's output alone, that its fixture is alive (alive_near / alive_exact: the floors are
written there).  The first copy lies LEAD = 41000 bases into the chromosome, beyond the largest max_frag used here (40000)
plus an end: nearer than that the mating is undefined (oracle/README.md) and no test here goes there.

Routes of the split launch (read off PeSet::append / admit, abm_pe_set.hpp, and emit_list, abm_pe_wave.hpp): in the seed
kernel a list may grow to seed_cap entries, and abm_ctx_set_pe_split refuses a seed_cap beyond 16384; a list that wants
more sets `overflow`, hence need_big, and the pair is the whole-pair kernel's.  A set that fills has 32768 > 16384 entries,
so under every split form a pair with a full set is counted in mapped_whole, never in mated_from_device_memory; a staging
area of 32768 entries cannot be asked for (test_a_staging_area_of_32768_entries_is_refused).

Seeded defects (each built into a copy of the library, this module run against it) and what catches them:
  the last radix pass gives a digit's lanes one slot too few, in lists of more than 20000 entries only: 24 tests fail --
      every one on `near`; the family without divergence and single-end pass (no long list is sorted there);
  worth forced true (a full set at cutoff 0 is mated all the same): the 8 tests of test_exact_family fail, nothing else;
  one sample in fifty of sample_list 300 bases too high when samp_shift >= 5: NOT caught -- a search then starts a
      mating window one or two entries early, a partner less than 300 bases beyond max_frag, which has to win or tie a
      pair to show.  Errors of an entry or two at a window's far edge are below what this fixture sees
      (test_gpu_pe_mating_steps.py runs the searches alone and catches it)."""
import concurrent.futures
import os

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_bam_records import check_pairs
from tests.test_gpu_diagnostic_builds import same_bytes, stamped
from tests.test_gpu_kernel_forms import expected_pe
from tests.test_gpu_pe_parity import compare_pe
from tests.test_gpu_pe_sam_text import check_text, same_results
from tests.test_gpu_pe_split import FORMS
from tests.test_gpu_se_parity import compare_se

pytestmark = pytest.mark.gpu

N_PAIRS = 64
N_READS = 256
COPIES, DIVERGENCE, LEAD = 30000, 0.025, 41000
MAXC = 30000
PE_CAP_LARGE = 32768    # kPeCapLarge
MAX_SEED_CAP = 16384    # abm_ctx_set_pe_split: "seed_cap: at most 16384"
GENOMES = {  # name -> (unit_len, divergence, iupac letters)
    "near": (200, DIVERGENCE, 0),
    "exact": (200, 0.0, 0),
    "near_iupac": (200, DIVERGENCE, 400),
    "near_400": (400, DIVERGENCE, 0),   # a unit of 400 bases, for ends of 200
}
WIDE, NARROW = dict(max_frag=40000), dict(min_frag=150, max_frag=300)


def by_mode(r1, r2, mode):
    """mode 1 (PBAT): the A-rich end comes first; mode 2 (random PBAT): in every other pair"""
    if mode == 1:
        return list(r2), list(r1)
    if mode == 2:
        return ([y if i % 2 else x for i, (x, y) in enumerate(zip(r1, r2))],
                [x if i % 2 else y for i, (x, y) in enumerate(zip(r1, r2))])
    return list(r1), list(r2)


def shares(orc):
    """(uniquely mapped, ambiguous, fallback hits only) pairs of an oracle result"""
    pairs, se1, se2 = orc[0], orc[1], orc[2]
    has = pairs["r1"]["pos"] != 0
    amb = has & ((pairs["r1"]["flags"] & 0x100) != 0)
    fallback = ~has & ((se1["pos"] != 0) | (se2["pos"] != 0))
    return int((has & ~amb).sum()), int(amb.sum()), int(fallback.sum())


def tallies(work):
    return {k: work[k] for k in ("pe_full_sets", "pe_lists_over_512", "pe_lists_over_4096", "pe_matings_skipped")}


def alive_near(orc, label):
    """floors on the oracle's output for the diverged family: sets fill, lists of thousands are sorted, a quarter of
    the pairs mapped as pairs without the ambiguity flag, an ambiguous pair, a pair with fallback hits only"""
    n, work = len(orc[0]), orc[5]
    unique, ambiguous, fallback = shares(orc)
    print(f"{label}: oracle: {tallies(work)}, {unique} unique, {ambiguous} ambiguous, {fallback} fallback-only of {n}")
    assert work["pe_full_sets"] > 0 and work["pe_lists_over_4096"] > 0, (label, tallies(work))
    assert 4 * unique >= n and ambiguous >= 1 and fallback >= 1, (label, unique, ambiguous, fallback)


def alive_exact(orc, mode, label):
    """floors for the family without divergence: sets full at cutoff 0 make the reference skip the mating; with two
    orientation calls per pair (mode 0) nothing is ever aligned"""
    work = orc[5]
    unique, ambiguous, fallback = shares(orc)
    print(f"{label}: oracle: {tallies(work)}, {unique} unique, {ambiguous} ambiguous, {fallback} fallback-only of {len(orc[0])}, "
          f"{work['aligns']} alignments")
    assert work["pe_full_sets"] > 0 and work["pe_matings_skipped"] > 0, (label, tallies(work))
    if mode == 0:
        assert work["aligns"] == 0, (label, work["aligns"])


class Bed:
    """one satellite genome, its index, the oracle's results (once per key) and one (index, context) per record size"""

    def __init__(self, oracle, workdir, name):
        unit, div, iupac = GENOMES[name]
        self.oracle, self.name = oracle, name
        self.fa = os.path.join(workdir, f"sat_{name}.fa")
        self.idx = os.path.join(workdir, f"sat_{name}.idx")
        self.lay = synth.satellite_genome(self.fa, COPIES, unit, div, LEAD, seed=5, iupac=iupac)
        oracle.index_build(self.fa, self.idx, threads=8)
        self.oix = oracle.index_load(self.idx)
        self._pairs, self._orc, self._ctx = {}, {}, {}

    def close(self):
        for ix, ctx in self._ctx.values():
            ctx.close()
            ix.close()
        self.oracle.index_free(self.oix)

    def ctx(self, window_records=None):
        import abismal_amd as A
        if window_records not in self._ctx:
            ix = A.Index(self.idx, window_records=window_records)
            self._ctx[window_records] = (ix, A.Context(ix, 0))
        ix, ctx = self._ctx[window_records]
        ctx.set_pe_split(-1)
        ctx.pe_split_stats()
        return ix, ctx

    def pairs(self, L, mode):
        if L not in self._pairs:
            # (exact: no planted differences either -- every end has thousands of perfect matches)
            self._pairs[L] = synth.pairs_on_satellite(self.lay, self.fa, N_PAIRS, L, seed=7, max_frag=WIDE["max_frag"],
                                                      planted=0.0 if self.name == "exact" else 0.5)
        return by_mode(*self._pairs[L], mode)

    def expected(self, L, mode, allow_ambig=False, **limits):
        key = (L, mode, allow_ambig, tuple(sorted(limits.items())))
        if key not in self._orc:
            r1, r2 = self.pairs(L, mode)
            self._orc[key] = self.oracle.map_pe(self.oix, r1, r2, mode=mode, max_candidates=MAXC, allow_ambig=allow_ambig, threads=16, **limits)
            label = f"{self.name} 2 x {L} mode {mode} {limits}"
            if self.name == "exact":
                alive_exact(self._orc[key], mode, label)
            else:
                alive_near(self._orc[key], label)
        return self._orc[key]

    def pairs_with_a_full_set(self, L):
        """how many pairs of the mode-0 batch fill a set, from the oracle's tally pair by pair"""
        if ("full", L) not in self._orc:
            r1, r2 = self.pairs(L, 0)
            with concurrent.futures.ThreadPoolExecutor(8) as pool:  # (the C call releases the interpreter lock)
                work = list(pool.map(lambda ab: self.oracle.map_pe(self.oix, [ab[0]], [ab[1]], mode=0, max_candidates=MAXC)[5], zip(r1, r2)))
            self._orc["full", L] = sum(1 for w in work if w["pe_full_sets"] > 0)
        return self._orc["full", L]


@pytest.fixture(scope="module")
def beds(oracle, workdir):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Bed(oracle, workdir, name)
        return made[name]

    yield get
    for b in made.values():
        b.close()


def params(allow_ambig=False, **limits):
    import abismal_amd as A
    return A.Params(max_candidates=MAXC, allow_ambig=1 if allow_ambig else 0, **limits)


# ---- 1. the whole-pair launch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_whole_pair_launch(beds, mode):
    bed = beds("near")
    orc = bed.expected(100, mode)
    r1, r2 = bed.pairs(100, mode)
    ix, ctx = bed.ctx()
    ctx.set_pe_split(split=0)
    compare_pe(ctx.map_pe(r1, r2, mode=mode, params=params()), orc, f"near, whole-pair launch, mode {mode}")
    st = ctx.pe_split_stats()
    assert st["mated_from_lds"] + st["mapped_whole"] + st["mated_from_device_memory"] == 0, st


# ---- 2. the split launch forms ---------------------------------------------------------------------------------------
SPLIT_CASES = [(form, 0) for form, _ in FORMS] + [("split_stage_16384", 2)]  # (16384: the largest staging area there is)


@pytest.mark.parametrize("form,mode", SPLIT_CASES, ids=[f"{f}-m{m}" for f, m in SPLIT_CASES])
def test_split_launch_forms(beds, form, mode):
    bed = beds("near")
    kw = dict(FORMS)[form]
    orc = bed.expected(100, mode)
    full = bed.pairs_with_a_full_set(100)
    assert full > 0
    r1, r2 = bed.pairs(100, mode)
    ix, ctx = bed.ctx()
    ctx.set_pe_split(**kw)
    ctx.pe_split_stats()
    compare_pe(ctx.map_pe(r1, r2, mode=mode, params=params()), orc, f"near, {form}, mode {mode}")
    st = ctx.pe_split_stats()
    print(f"near, {form}, mode {mode}: {st}; {full} pairs fill a set in mode 0")
    routed = st["mated_from_lds"] + st["mapped_whole"] + st["mated_from_device_memory"]
    if kw["split"] == 0:
        assert routed == 0, st
        return
    assert routed == len(r1), st
    # the rule in the module's docstring: a set that fills outgrew every staging area on its way, so its pair is mapped
    # whole.  (Mode 2 makes the calls of mode 0 and two more: a pair that fills a set in mode 0 does so in mode 2.)
    assert kw.get("seed_cap", 0) <= MAX_SEED_CAP
    assert st["mapped_whole"] >= full, (st, full)
    assert st["mated_from_device_memory"] <= len(r1) - full, (st, full)


def test_a_staging_area_of_32768_entries_is_refused(beds):
    """no split form hands a full set over: seed_cap = 32768 is refused, the form in force stays"""
    import abismal_amd as A
    bed = beds("near")
    orc = bed.expected(100, 0)
    r1, r2 = bed.pairs(100, 0)
    ix, ctx = bed.ctx()
    ctx.set_pe_split(split=1, seed_cap=MAX_SEED_CAP, hand_entries=24_000_000)
    with pytest.raises(A.AbismalAmdError, match="seed_cap"):
        ctx.set_pe_split(split=1, seed_cap=PE_CAP_LARGE, hand_entries=8 * N_PAIRS * PE_CAP_LARGE)
    ctx.pe_split_stats()
    compare_pe(ctx.map_pe(r1, r2, mode=0, params=params()), orc, "near, after the refused form")
    st = ctx.pe_split_stats()
    assert st["mated_from_lds"] + st["mapped_whole"] + st["mated_from_device_memory"] == len(r1), st


# ---- 3. fragment limits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limits", [WIDE, NARROW], ids=["L40000", "l150_L300"])
@pytest.mark.parametrize("mode", [0, 2])
def test_fragment_limits(beds, mode, limits):
    """copies every 220 bases: max_frag 40000 gives a list-1 entry about 180 partners, a window of three 64-step chunks
    (mate's carry / seen / prev_hi); 150-300 gives it one or two"""
    bed = beds("near")
    orc = bed.expected(100, mode, **limits)
    r1, r2 = bed.pairs(100, mode)
    ix, ctx = bed.ctx()
    for split in (0, -1):
        ctx.set_pe_split(split=split)
        compare_pe(ctx.map_pe(r1, r2, mode=mode, params=params(**limits)), orc, f"near, {limits}, mode {mode}, split {split}")


# ---- 4. every filter -------------------------------------------------------------------------------------------------
FILTER_CASES = [  # (genome, end length, window records asked for, filter form, records served)
    ("near", 100, None, "records", 172),     # the record-fed seed kernel
    ("near", 150, 0, "planes", 0),           # bit planes, four-lane groups
    ("near_400", 200, None, "planes", 172),  # eight-lane groups (records for 172 bases do not serve ends of 200)
    ("near_iupac", 100, None, "nibbles", 0), # one lane per window on the nibble array
]


@pytest.mark.parametrize("genome,L,asked,flt,serves", FILTER_CASES, ids=[f"{g}-2x{L}-{f}" for g, L, _, f, _ in FILTER_CASES])
def test_every_filter(beds, genome, L, asked, flt, serves):
    bed = beds(genome)
    orc = bed.expected(L, 0)
    r1, r2 = bed.pairs(L, 0)
    assert max(len(x) for x in r1 + r2) == L
    ix, ctx = bed.ctx(asked)
    assert ctx.window_records() == serves and ctx.filter_on_planes() == (flt != "nibbles")
    for split in (0, -1):
        ctx.set_pe_split(split=split)
        compare_pe(ctx.map_pe(r1, r2, mode=0, params=params()), orc, f"{genome} 2 x {L}, {flt}, split {split}")
        launched = ctx.last_forms(lds=True)
        lds_of = {(f.phase, f.big): lds for f, lds in launched}
        assert [f for f, _ in launched] == expected_pe(split != 0, flt, False, None, lds_of), (genome, L, split, launched)


# ---- 5. records written by the kernels -------------------------------------------------------------------------------
@pytest.mark.parametrize("allow_ambig", [False, True])
@pytest.mark.parametrize("split", [0, -1], ids=["whole", "split"])
def test_device_written_records(beds, split, allow_ambig):
    """SAM text and BAM pieces from the text builds of the whole-pair kernel on full sets.  No end beyond 1,024 bases and
    no CIGAR beyond 50 ops in this fixture, so -- as in tests/test_gpu_pe_filter_paths.py -- at least 98 % of the pairs
    must come with the device's records."""
    bed = beds("near")
    orc = bed.expected(100, 0, allow_ambig=allow_ambig)
    r1, r2 = bed.pairs(100, 0)
    ix, ctx = bed.ctx()
    ctx.set_pe_split(split=split)
    p = params(allow_ambig)
    label = f"near, split {split}, allow_ambig {allow_ambig}"
    plain = ctx.map_pe(r1, r2, mode=0, params=p)
    compare_pe(plain, orc, label)
    ctx.set_sam_tails(True, allow_ambig=allow_ambig)
    try:
        text = ctx.map_pe(r1, r2, mode=0, params=p, sam=True)
        ctx.set_record_format(bam=True)
        pieces = ctx.map_pe(r1, r2, mode=0, params=p, sam=True)
    finally:
        ctx.set_sam_tails(False)
        ctx.set_record_format(bam=False)
    same_results(plain, text, label + ", SAM text")
    same_results(plain, pieces, label + ", BAM pieces")
    check_text(ix, r1, r2, text, allow_ambig, label, min_device=0.98)
    check_pairs(ix, r1, r2, pieces, allow_ambig, label, 0.98)


# ---- 6. the diagnostic build -----------------------------------------------------------------------------------------
def test_diagnostic_build(beds):
    """results byte for byte those of the production build; the per-pair word (largest set << 16 | cycles >> 20) shows a
    set of 32768 entries; tier 2 spent cycles in sort_unique"""
    import torch
    bed = beds("near")
    orc = bed.expected(100, 0)
    r1, r2 = bed.pairs(100, 0)
    n = len(r1)
    ix, ctx = bed.ctx()
    ctx.set_pe_split(split=0)
    plain = ctx.map_pe(r1, r2, mode=0, params=params())
    words = torch.zeros((n + 64,), dtype=torch.int32, device="cuda")
    ctx.set_read_cycles(words.data_ptr())
    try:
        diag, (t1, t2) = stamped(ctx, lambda: ctx.map_pe(r1, r2, mode=0, params=params()))
        torch.cuda.synchronize()
        sets = words.cpu().numpy()[:n].view(np.uint32) >> 16
    finally:
        ctx.set_read_cycles(None)
    same_bytes(plain, diag, "near, diagnostic build")
    compare_pe(diag, orc, "near, diagnostic build")
    print(f"near, diagnostic build: largest set {sets.max()}, pairs with a set of {PE_CAP_LARGE}: {(sets == PE_CAP_LARGE).sum()}, tier 2: {t2}")
    assert sets.max() == PE_CAP_LARGE and (sets == PE_CAP_LARGE).sum() == bed.pairs_with_a_full_set(100)
    assert t2["cyc_sort_unique"] > 0 and t2["cyc_total"] > 0, t2


# ---- 7. the family without divergence --------------------------------------------------------------------------------
@pytest.mark.parametrize("allow_ambig", [False, True])
@pytest.mark.parametrize("split", [0, -1], ids=["whole", "split"])
@pytest.mark.parametrize("mode", [0, 2])
def test_exact_family(beds, mode, split, allow_ambig):
    """every set full at cutoff 0: worth == false, no mating, heap_order_now on the lists still in arrival order, both
    ends reported from the best-single log; sure_ambig stops the seed passes"""
    bed = beds("exact")
    orc = bed.expected(100, mode, allow_ambig=allow_ambig)
    r1, r2 = bed.pairs(100, mode)
    ix, ctx = bed.ctx()
    ctx.set_pe_split(split=split)
    compare_pe(ctx.map_pe(r1, r2, mode=mode, params=params(allow_ambig)), orc, f"exact, mode {mode}, split {split}, allow_ambig {allow_ambig}")


# ---- 8. single-end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("genome", ["near", "exact"])
@pytest.mark.parametrize("mode", [0, 2])
def test_single_end(beds, genome, mode):
    """256 reads of 100 bases, three in ten of them cut to 47-99: flattened blocks of tens of thousands of candidates go
    through locate128 and the heavy-read priority path"""
    bed = beds(genome)
    reads = synth.reads_on_satellite(bed.lay, bed.fa, N_READS, 100, seed=11)
    assert sum(1 for r in reads if len(r) < 100) > N_READS // 5 and max(len(r) for r in reads) == 100
    o_res, o_cig, o_n, work = bed.oracle.map_se(bed.oix, reads, mode=mode, max_candidates=MAXC, threads=16)
    mapped, ambiguous = int((o_res["pos"] != 0).sum()), int(((o_res["pos"] != 0) & ((o_res["flags"] & 0x100) != 0)).sum())
    print(f"{genome} single-end mode {mode}: oracle maps {mapped} of {len(reads)}, {ambiguous} of them ambiguous; "
          f"{work['candidates']} candidates")
    assert work["candidates"] > COPIES // 3 * len(reads), "the reads do not meet the family's copies by the ten thousand"
    assert mapped > N_READS // 2 and (ambiguous > 0 if genome == "exact" else mapped - ambiguous >= N_READS // 4)
    ix, ctx = bed.ctx()
    res, cig, off = ctx.map_se(reads, mode=mode, params=params())
    compare_se(res, cig, off, o_res, o_cig, o_n, reads, f"{genome} single-end mode {mode}")
