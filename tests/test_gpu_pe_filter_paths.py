"""GPU parity of the paired-end path across every Hamming filter its launches choose from, and every end length that
switches between them.  abm_map_pe_device (abm_api.hip) takes the batch's longest end, at most 1,024 bases, as eff_len
and sets G = 4 for eff_len <= 192, 8 for eff_len <= 448, 0 beyond that or when the genome has no bit planes (IUPAC
letters); pe_select() (abm_kernel_form.hpp) then picks

    G == 4 and window records that serve eff_len (108 / 140 / 172)   the record-fed seed kernel (REC)
    G == 4 otherwise                                                 bit planes, four-lane groups
    G == 8                                                           bit planes, eight-lane groups
    G == 0                                                           one lane per window on the nibble array (COOP = false)

and ends beyond 1,024 bases get the long-end launch on top (tests/test_gpu_edges_and_properties.py).  Here: uniform, ragged
and unequal ends either side of every switch, every record size and none, the launch forms off the records, a genome with
IUPAC letters, pairs at the edges of N runs through each filter, a batch-composition property, and the SAM text of the plane
builds beyond 150 bases.  Pair, both fallback hits and both CIGARs equal the oracle's, bit for bit (compare_pe); every
test first asserts on the ORACLE's output that its fixture is alive (pairs mapped, probes made, a pair with fallback hits only)
and on the context that the path it names is the one selected."""
import os
import zlib

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_pe_parity import compare_pe
from tests.test_gpu_pe_sam_text import check_text, mapped_twice, same_results
from tests.test_gpu_pe_split import FORMS

pytestmark = pytest.mark.gpu

N_PAIRS = 2000  # (pairs per input; the module then costs 2.7 s a test, about what the rest of the GPU suite does: DESIGN.md, section 2)
SWITCH_LENGTHS = (150, 172, 173, 192, 193, 250, 448, 449, 700, 1024)
RECORD_SIZES = ((0, 0), (100, 108), (109, 140), (150, 172))  # (asked for, serves)


def u(L):
    return ("uniform", L)


def ragged(L):
    return ("ragged", L)


def unequal(L1, L2):
    return ("unequal", L1, L2)


def name(spec):
    return spec[0] + "_" + "_".join(str(x) for x in spec[1:])


class Bed:
    """one genome, its index, the inputs cut from it and the oracle's results for them (once per input and mode), and one
    context per record size"""

    def __init__(self, oracle, fa, idx):
        self.oracle, self.fa, self.idx = oracle, fa, idx
        self.oix = oracle.index_load(idx)
        self._pairs, self._orc, self._ctx = {}, {}, {}

    def close(self):
        for ix, ctx in self._ctx.values():
            ctx.close()
            ix.close()
        self.oracle.index_free(self.oix)

    def ctx(self, window_records=None):
        """(index, context) with records asked for reads of that length (None: the suite's default, 172)"""
        import abismal_amd as A
        if window_records not in self._ctx:
            ix = A.Index(self.idx, window_records=window_records)
            self._ctx[window_records] = (ix, A.Context(ix, 0))
        return self._ctx[window_records]

    def pairs(self, spec, mode, n=N_PAIRS):
        """mode 1 (PBAT): the A-rich end comes first; mode 2 (random PBAT): in every other pair"""
        key = (spec, mode, n)
        if key in self._pairs:
            return self._pairs[key]
        kind = spec[0]
        top = max(spec[1:])
        frag = (120, 900) if top <= 448 else (top + 12, 1100)
        seed = zlib.crc32(name(spec).encode())  # (one seed per input; the three modes share the fragments)
        r1, r2 = synth.mutated_pairs(self.fa, n, top, seed=seed, frag=frag)
        if kind == "ragged":
            r1, r2 = synth.cut_pairs_ragged(r1, r2, np.random.default_rng(seed + 1), 44, top)
        elif kind == "unequal":
            r1, r2 = synth.cut_pairs_fixed(r1, r2, *spec[1:])
        r1, r2 = synth.trim_like_readloader(r1), synth.trim_like_readloader(r2)
        if mode == 1:
            r1, r2 = r2, r1
        elif mode == 2:
            for k in range(1, len(r1), 2):
                r1[k], r2[k] = r2[k], r1[k]
        assert max(len(x) for x in r1 + r2) == top, "the batch's longest end selects the filter"
        self._pairs[key] = (r1, r2)
        return r1, r2

    def map_oracle(self, r1, r2, mode, **kw):
        # (ends of 44-46 bases see what the ends before them left behind, in input order: one thread, as the single-end tests do)
        short = any(44 <= len(x) <= 46 for x in r1 + r2)
        return self.oracle.map_pe(self.oix, r1, r2, mode=mode, threads=1 if short else 8, **kw)

    def expected(self, spec, mode, n=N_PAIRS):
        """the oracle's result for pairs(spec, mode), checked for liveness"""
        key = (spec, mode, n)
        if key not in self._orc:
            r1, r2 = self.pairs(spec, mode, n)
            orc = self.map_oracle(r1, r2, mode)
            alive(orc, f"{name(spec)} mode {mode}")
            self._orc[key] = orc
        return self._orc[key]


def alive(orc, label, floor=0.8):
    """the fixture-liveness floors, on the oracle's output: pairs mapped, probes made, a pair with fallback hits only"""
    pairs, se1, se2, work = orc[0], orc[1], orc[2], orc[5]
    mapped = float((pairs["r1"]["pos"] != 0).mean())
    fallback_only = int(((pairs["r1"]["pos"] == 0) & ((se1["pos"] != 0) | (se2["pos"] != 0))).sum())
    print(f"{label}: oracle maps {mapped:.3f} of {len(pairs)} pairs, {fallback_only} with fallback hits only, "
          f"{work['search_probes']} probes")
    assert mapped > floor, f"{label}: the oracle maps only {mapped:.3f} of the pairs"
    assert work["search_probes"] > 0, label
    assert fallback_only >= 1, f"{label}: no pair with fallback hits only"


@pytest.fixture(scope="module")
def bed(oracle, workdir):
    import abismal_amd as A
    fa = os.path.join(workdir, "rep_pe_paths.fa")
    idx = os.path.join(workdir, "rep_pe_paths.idx")
    synth.repeat_rich_genome(fa)
    A.index_build(fa, idx, 8)
    b = Bed(oracle, fa, idx)
    yield b
    b.close()


@pytest.fixture(scope="module")
def iupac_bed(oracle, workdir):
    import abismal_amd as A
    fa = os.path.join(workdir, "iupac_pe_paths.fa")
    idx = os.path.join(workdir, "iupac_pe_paths.idx")
    synth.repeat_rich_genome(fa, seed=21, n_chroms=2, chrom_len=600_000, iupac=6000)
    A.index_build(fa, idx, 8)
    b = Bed(oracle, fa, idx)
    yield b
    b.close()


# ---- 1. end lengths around every switch of the pair launch -----------------------------------------------------------
# (the ten lengths either side of the switches in mode 0; 180, 250 and 449 -- one per plane / nibble filter -- in all three modes)
SWITCH_CASES = [(L, 0) for L in SWITCH_LENGTHS] + [(180, 0)] + [(L, m) for m in (1, 2) for L in (180, 250, 449)]


@pytest.mark.parametrize("shape", [u, ragged], ids=["uniform", "ragged"])
@pytest.mark.parametrize("L,mode", SWITCH_CASES)
def test_end_lengths_around_every_switch(bed, L, mode, shape):
    """The default index (records that serve 172 bases); longest end of the batch, by the launch rule above (eff_len = L):
    150, 172: the record-fed seed kernel; 173, 180, 192: bit planes, four-lane groups (G = 4, records too short);
    193, 250, 448: bit planes, eight-lane groups (G = 8); 449, 700, 1024: one lane per window on the nibble array (G = 0).
    One uniform batch, and one ragged batch with both ends of every pair cut independently to 44 ... L bases and the last
    pair whole (lane groups, LDS sizes and the per-end lengths all come from the batch's longest end)."""
    ix, ctx = bed.ctx()
    assert ctx.window_records() == 172 and ctx.filter_on_planes()
    r1, r2 = bed.pairs(shape(L), mode)
    orc = bed.expected(shape(L), mode)
    compare_pe(ctx.map_pe(r1, r2, mode=mode), orc, f"{name(shape(L))} mode {mode}, records for 172")


# ---- 2. every record size, and none ----------------------------------------------------------------------------------
RECORD_INPUTS = [u(L) for L in (100, 108, 109, 140, 150, 172)] + [ragged(172), unequal(100, 172), unequal(172, 100)]


@pytest.mark.parametrize("spec", RECORD_INPUTS, ids=name)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_record_size_and_none(bed, mode, spec):
    """window records asked for 0 / 100 / 109 / 150 bases serve 0 / 108 / 140 / 172 (records of three, four and five blocks):
    each size gets batches it serves (the record-fed seed kernel) and batches it does not (the planes, four-lane groups)."""
    r1, r2 = bed.pairs(spec, mode)
    orc = bed.expected(spec, mode)
    for asked, serves in RECORD_SIZES:
        ix, ctx = bed.ctx(asked)
        assert ctx.window_records() == serves and ctx.filter_on_planes()
        compare_pe(ctx.map_pe(r1, r2, mode=mode), orc, f"{name(spec)} mode {mode}, records for {serves}")


# ---- 3. the launch forms off the records -----------------------------------------------------------------------------
@pytest.mark.parametrize("asked,serves,L,mode", [(0, 0, 100, 0), (None, 172, 250, 0), (None, 172, 250, 2)])
def test_launch_forms_off_the_records(bed, asked, serves, L, mode):
    """tests/test_gpu_pe_split.py's forms where the seed kernel is not record-fed: 2 x 100 on an index without records
    (planes, four-lane groups) and 2 x 250 (eight-lane groups); over the forms every route is taken."""
    import abismal_amd as A
    r1, r2 = bed.pairs(u(L), mode)
    orc = bed.expected(u(L), mode)
    ix = A.Index(bed.idx, window_records=asked)
    ctx = A.Context(ix, 0)
    routes = {"mated_from_lds": 0, "mapped_whole": 0, "mated_from_device_memory": 0}
    try:
        assert ctx.window_records() == serves and ctx.filter_on_planes()
        for form, kw in FORMS:
            ctx.set_pe_split(**kw)
            ctx.pe_split_stats()
            compare_pe(ctx.map_pe(r1, r2, mode=mode), orc, f"2 x {L} mode {mode}, records for {serves}, {form}")
            st = ctx.pe_split_stats()
            routed = sum(st[k] for k in routes)
            assert routed == (len(r1) if kw["split"] else 0), (form, st)
            for k in routes:
                routes[k] += st[k]
    finally:
        ctx.close()
        ix.close()
    assert all(v > 0 for v in routes.values()), routes


# ---- 4. pairs on a genome with IUPAC letters -------------------------------------------------------------------------
@pytest.mark.parametrize("L", [100, 150, 250])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pairs_on_an_iupac_genome(iupac_bed, mode, L):
    """A genome with IUPAC letters has no bit planes and gets no window records: the pair kernels run one lane per window on
    the nibble array at every end length, and size their alignment windows with size_frac = 1.0.  Such launches write no SAM
    text (abm_ctx_pe_sam_tails: the batch is the host's), and asking for it changes no result."""
    ix, ctx = iupac_bed.ctx()
    assert not ctx.filter_on_planes() and ctx.window_records() == 0
    r1, r2 = iupac_bed.pairs(u(L), mode)
    orc = iupac_bed.expected(u(L), mode)
    plain, text = mapped_twice(ctx, r1, r2, mode, False)
    compare_pe(plain, orc, f"IUPAC genome, 2 x {L} mode {mode}")
    assert text[5] is None and text[6] is None
    same_results(plain, text, f"IUPAC genome, 2 x {L} mode {mode}")


# ---- 5. pairs at the edges of N runs, per filter ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def n_run_bed(oracle, workdir):
    fa = os.path.join(workdir, "nrun_pe_paths.fa")
    idx = os.path.join(workdir, "nrun_pe_paths.idx")
    synth.repeat_rich_genome(fa, seed=11, n_chroms=2, chrom_len=400_000)
    oracle.index_build(fa, idx, threads=4)
    b = Bed(oracle, fa, idx)
    yield b
    b.close()


@pytest.mark.parametrize("L", [100, 150, 250, 300])
def test_pairs_at_the_edges_of_n_runs(n_run_bed, L):
    """One end cut at distance 0 ... 24 from the long N run, either side of it, either strand, either end; pairs whose
    ends lie on the two sides of the short, LCG-filled run; and pairs with one end at the long run and the other too far
    away to be its mate, which give the fixture its pairs with fallback hits only (exact pairs alone have none).  The
    record-fed kernel's narrowing probes read letters from the records and go to the nibble array where a record's N flag
    is set; without records (or with records too short: 108 for ends of 150) the probes and the four-lane filter read the
    planes, and ends of 250 and 300 take eight-lane groups.
    These ends stop before the run and no repeat lies against it, so no bucket that is narrowed (more than max_candidates
    entries) holds an entry whose probed letters lie inside the run: this test guards the filters and the lane groups at
    the runs' edges.  The narrowing probes' way back to the nibble array (record_nibble where a record's N flag is set,
    narrow_direct's `ok`) is reached by tests/test_gpu_narrowing_at_n_runs.py: tests/hip/narrow_check.hip on the
    functions themselves, and a repeat family with copies cut short by N runs end to end."""
    b = n_run_bed
    r1, r2 = synth.pairs_at_n_runs(synth.read_chroms(b.fa), (L,), seed=4 + L, mirrored=True, straddle=True, unmated=True)
    orc = b.map_oracle(r1, r2, 0)
    alive(orc, f"pairs at the edges of N runs, 2 x {L}")
    for asked, serves in ((0, 0), (100, 108), (172, 172)):
        ix, ctx = b.ctx(asked)
        assert ctx.window_records() == serves and ctx.filter_on_planes()
        compare_pe(ctx.map_pe(r1, r2), orc, f"pairs at the edges of N runs, 2 x {L}, records for {serves}")


# ---- 6. batch composition does not change a pair's result ------------------------------------------------------------
def test_batch_composition_does_not_matter(bed):
    """One longer pair appended to a batch of 2 x 100 moves every other pair from the record-fed kernel to the planes with
    four-lane groups (180), with eight-lane groups (300), to the nibble array (500), and to the nibble array at eff_len
    1,024 beside the long-end launch (1,100): their pair records, fallback hits and CIGARs stay byte for byte what they
    were, split or not; the appended pair equals the oracle's.  (No end of this batch has 44-46 bases -- mutated_pairs cuts
    an end to 100 or to 30 -- so no result depends on what the ends before it left behind; were there one, appending, not
    prepending, the extra pair keeps what comes before every pair the same.)"""
    import abismal_amd as A
    n = 1500
    r1, r2 = bed.pairs(u(100), 0, n)
    orc = bed.map_oracle(r1, r2, 0)
    alive(orc, "2 x 100, 1500 pairs")
    extra = {}
    for L in (180, 300, 500, 1100):
        a, b = synth.mutated_pairs(bed.fa, 1, L, seed=77 + L, frag=(L + 12, L + 300))
        a, b = synth.trim_like_readloader(a), synth.trim_like_readloader(b)
        assert max(len(a[0]), len(b[0])) == L
        o = bed.map_oracle(a, b, 0)
        assert int(o[0]["r1"]["pos"][0]) != 0, f"the oracle must map the appended pair of 2 x {L}"
        extra[L] = (a, b, o)
    ix = A.Index(bed.idx)
    ctx = A.Context(ix, 0)

    def head(g):
        pairs, se1, se2, (c1, o1), (c2, o2) = g[:5]
        return (pairs[:n].tobytes(), se1[:n].tobytes(), se2[:n].tobytes(), c1[:int(o1[n])].tobytes(), o1[:n + 1].tobytes(),
                c2[:int(o2[n])].tobytes(), o2[:n + 1].tobytes())

    def last(g):
        pairs, se1, se2, (c1, o1), (c2, o2) = g[:5]
        z = np.zeros(1, dtype=np.uint64)
        return (pairs[n:], se1[n:], se2[n:], (c1[int(o1[n]):], np.concatenate([z, o1[n + 1:] - o1[n]])),
                (c2[int(o2[n]):], np.concatenate([z, o2[n + 1:] - o2[n]])))

    try:
        assert ctx.window_records() == 172 and ctx.filter_on_planes()
        alone = ctx.map_pe(r1, r2)
        compare_pe(alone, orc, "2 x 100 alone")
        for split in (-1, 0):
            ctx.set_pe_split(split=split)
            assert head(ctx.map_pe(r1, r2)) == head(alone), f"2 x 100 alone, split {split}"
            for L, (a, b, o) in extra.items():
                g = ctx.map_pe(r1 + a, r2 + b)
                same = [x == y for x, y in zip(head(g), head(alone))]
                assert all(same), f"a pair of 2 x {L} appended, split {split}: (pairs, se1, se2, cig1, off1, cig2, off2) same: {same}"
                compare_pe(last(g), o, f"the appended pair of 2 x {L}, split {split}")
    finally:
        ctx.close()
        ix.close()


# ---- 7. SAM text from the plane builds beyond 150 bases --------------------------------------------------------------
@pytest.mark.parametrize("spec", [u(180), u(250), u(448), unequal(100, 250)], ids=name)
@pytest.mark.parametrize("mode", [0, 2])
def test_sam_text_beyond_150_bases(bed, mode, spec):
    """The text builds run on the bit planes at every end length up to 448, records or not: four-lane groups at 180,
    eight-lane groups at 250 and 448.  Every pair's records equal tests/sam_format.py byte for byte and results are those
    of the text-off call; no pair of the fixture has an end beyond 1,024 bases or a CIGAR beyond 50 ops, so at least 98 %
    of the pairs must come with the device's text."""
    r1, r2 = bed.pairs(spec, mode)
    orc = bed.expected(spec, mode)
    for asked, serves in ((None, 172), (0, 0)):
        ix, ctx = bed.ctx(asked)
        assert ctx.window_records() == serves and ctx.filter_on_planes()
        for allow_ambig in (False, True):
            label = f"{name(spec)} mode {mode}, records for {serves}, allow_ambig {allow_ambig}"
            plain, text = mapped_twice(ctx, r1, r2, mode, allow_ambig)
            same_results(plain, text, label)
            if not allow_ambig:
                compare_pe(plain, orc, label)
            check_text(ix, r1, r2, text, allow_ambig, label, min_device=0.98)


def test_no_text_beyond_448_bases(bed):
    """a batch whose longest end is 449 bases is filtered on the nibble array, whose builds write no text: none comes back,
    and asking for it changes no result"""
    ix, ctx = bed.ctx()
    r1, r2 = bed.pairs(u(449), 0)
    orc = bed.expected(u(449), 0)
    plain, text = mapped_twice(ctx, r1, r2, 0, False)
    assert text[5] is None and text[6] is None
    same_results(plain, text, "2 x 449")
    compare_pe(plain, orc, "2 x 449")
