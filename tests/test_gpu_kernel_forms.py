"""Which build of the mapping kernels each launch route takes (abm_kernel_form.hpp: the tables and pe_select / se_select), as the
context reports it (Context.last_forms), and that every build computes what the oracle does.

Every case maps one small batch, asserts that the reported forms are exactly the ones the route, the index's filter, the
stamps and the records asked for call for, and compares the results with the oracle's (compare_se / compare_pe).  A refused
combination launches nothing that would fail: the text stride comes back 0 (no records are returned) and the reported forms
are the text-less ones -- BAM pieces with the stamps on (single-end), text with the stamps on and text without bit planes
(pairs).

Three waves per SIMD: pe_select gives a whole-pair launch on the planes the 3-wave build when 160 KB / (LDS per wave) <= 13.
The expectation takes the LDS per wave the context reports for that launch, and each case asserts on which side of the
threshold it lies: 2x100 below for both tiers, 2x150 above for tier 1 alone, 2x172 above for both.

The union of the forms reported over this module is all 42 builds (test_every_build_ran, last in the file): none is out
of reach at this scale, so the list of unreachable forms (at most four are allowed) is empty."""
import os

import pytest

from abismal_amd.api import PeForm, SeForm
from tests import oracle_binding as ob
from tests import synth
from tests.test_gpu_diagnostic_builds import beds, filter_ctx  # noqa: F401  (beds: a fixture)
from tests.test_gpu_pe_parity import compare_pe, sim_pairs
from tests.test_gpu_pe_split import FORMS
from tests.test_gpu_se_parity import compare_se

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (a hand-over area of 64 entries: no list finds room, every pair goes the whole-pair way, the mate kernels still launch)
ROUTES = FORMS + [("split_area_64", dict(split=1, seed_cap=16384, hand_entries=64))]
BED_OF = {"planes": "rep", "records": "rep", "nibbles": "iupac"}
SEEN = set()
LDS_PER_CU = 160 * 1024


def three_waves(lds):
    return lds != 0 and LDS_PER_CU // lds <= 13


def expected_pe(split, flt, stamps, text, lds_of):
    """text: None, "sam" or "bam" -- what the batch writes (None as well where it is refused); lds_of: phase, big -> the
    reported LDS bytes of that launch"""
    coop, rec = flt != "nibbles", flt == "records"

    def whole(big):
        wps = 3 if coop and not stamps and not text and three_waves(lds_of["whole", big]) else 4
        return PeForm("whole", big, False, stamps, coop, rec and big and not text, text is not None, text == "bam", wps)

    def mate(big):
        return PeForm("mate", big, False, stamps, False, False, text is not None, text == "bam", 4)

    if not split:
        return [whole(False), whole(True)]
    return [PeForm("seed", False, False, stamps, coop, rec, False, False, 4), mate(False), mate(True), whole(True)]


def with_records(ctx, text, fn):
    """fn() with the kernels asked for SAM text or BAM pieces (text: None, "sam", "bam")"""
    if text is None:
        return fn()
    ctx.set_sam_tails(True)
    ctx.set_record_format(bam=text == "bam")
    try:
        return fn()
    finally:
        ctx.set_sam_tails(False)
        ctx.set_record_format(bam=False)


def run_pe(ctx, r1, r2, mode, flt, split, stamps, text, label):
    """one paired batch through the host entry point; its forms asserted; returns (results, {(phase, big): LDS bytes})"""
    ctx.set_phase_stamps(stamps)
    try:
        out = with_records(ctx, text, lambda: ctx.map_pe(r1, r2, mode=mode, sam=text is not None))
    finally:
        ctx.set_phase_stamps(False)
    launched = ctx.last_forms(lds=True)
    lds_of = {(f.phase, f.big): lds for f, lds in launched}
    written = text if (text and not stamps and flt != "nibbles") else None  # (refused: with the stamps, without planes)
    got = [f for f, _ in launched]
    assert got == expected_pe(split, flt, stamps, written, lds_of), f"{label}: {launched}"
    if text is not None:
        assert (out[5] is not None) == (written is not None), f"{label}: records {'missing' if written else 'written'}"
    SEEN.update(got)
    return out[:5], lds_of


PE_CASES = [(flt, 100, route) for flt in ("planes", "records", "nibbles") for route, _ in ROUTES] + \
           [(flt, L, route) for flt in ("planes", "records", "nibbles") for L in (150, 172) for route in ("unsplit", "split")]


@pytest.mark.parametrize("flt,L,route", PE_CASES, ids=[f"{f}-2x{L}-{r}" for f, L, r in PE_CASES])
def test_pe_forms_by_route(beds, flt, L, route):
    """200 pairs on the repeat-rich genome (planes; with window records for ends of up to 172 bases) or its copy with IUPAC
    letters (nibble array), by launch route, with the stamps off and on, writing nothing, SAM text and BAM pieces"""
    bed = beds(BED_OF[flt])
    ctx = filter_ctx(bed, flt)
    kw = dict(ROUTES)[route]
    mode = (PE_CASES.index((flt, L, route))) % 3
    r1, r2 = bed.pairs(mode, L, 200)
    assert max(len(r) for r in r1 + r2) == L
    orc = bed.expected_pe(r1, r2, mode, ("forms", mode, L))
    ctx.set_pe_split(**kw)
    for stamps in (False, True):
        for text in (None, "sam", "bam"):
            label = f"{flt} 2x{L} {route} mode {mode} stamps {stamps} text {text}"
            out, lds_of = run_pe(ctx, r1, r2, mode, flt, kw["split"] != 0, stamps, text, label)
            compare_pe(out, orc, label)
            if text is None and flt != "nibbles":  # the threshold's side, from the LDS the library computed for the launch
                assert three_waves(lds_of["whole", True]) == (L >= 172), (label, lds_of)
                if not kw["split"]:
                    assert three_waves(lds_of["whole", False]) == (L >= 150), (label, lds_of)


def expected_se(flt, G, stamps, bam):
    rec = flt == "records" and G in (2, 4)
    return SeForm(stamps, flt != "nibbles", rec, bam, False, 5)


def run_se(ctx, reads, mode, flt, G, stamps, text, label, long_reads=False):
    """text None: abm_map_se_batch; "sam" / "bam": the sliced entry point with records asked for"""
    cuts = [0, len(reads) // 3, len(reads)]
    ctx.set_phase_stamps(stamps)
    try:
        if text is None:
            out = ctx.map_se(reads, mode=mode)
        else:
            out = with_records(ctx, text, lambda: ctx.map_se_sliced(reads, cuts, mode=mode, tails=True))
    finally:
        ctx.set_phase_stamps(False)
    got = ctx.last_forms()
    refused = text == "bam" and stamps  # (no stamped build writes BAM pieces)
    want = [expected_se(flt, G, stamps, text == "bam" and not refused)] + ([SeForm(False, False, False, False, True, 1)] if long_reads else [])
    assert got == want, f"{label}: {got}"
    if text is not None:
        tails = out[4]
        if refused:
            assert all(t is None for t in tails), f"{label}: records written"
        else:
            assert any(tails), f"{label}: no records written"
    SEEN.update(got)
    return out[:3]


SE_CASES = [(flt, L) for flt in ("planes", "records", "nibbles") for L in (100, 150)]


@pytest.mark.parametrize("flt,L", SE_CASES, ids=[f"{f}-L{L}" for f, L in SE_CASES])
def test_se_forms(beds, flt, L):
    """300 reads (two lanes per window at 100 bases, four at 150), stamps off and on, no records, SAM text and BAM pieces"""
    bed = beds(BED_OF[flt])
    ctx = filter_ctx(bed, flt)
    mode = SE_CASES.index((flt, L)) % 3
    reads = bed.reads(mode, L, 300)
    assert max(len(r) for r in reads) == L
    o_res, o_cig, o_n, _ = bed.expected_se(reads, mode, ("forms", mode, L))
    for stamps in (False, True):
        for text in (None, "sam", "bam"):
            label = f"SE {flt} L {L} mode {mode} stamps {stamps} text {text}"
            out = run_se(ctx, reads, mode, flt, 0 if flt == "nibbles" else (2 if L <= 128 else 4), stamps, text, label)
            compare_se(*out, o_res, o_cig, o_n, reads, label)


def long_pieces(fa, n, L=1100):
    """n (forward piece, reverse-complemented piece 300 bases downstream) of L bases each, C -> T, off chromosome 1"""
    chrom = bytes(synth.read_chroms(fa)[0]).decode().upper()
    comp = str.maketrans("ACGT", "TGCA")
    out = []
    for k in range(n):
        p = 3000 + 7001 * k
        frag = chrom[p:p + 2 * L + 300]
        out.append((frag[:L].replace("C", "T"), frag[-L:][::-1].translate(comp).replace("C", "T")))
    return out


@pytest.mark.parametrize("stamps", [False, True], ids=["plain", "stamped"])
def test_long_forms(beds, oracle, stamps):
    """8 reads / 4 pairs of 1100 bases among ordinary ones: a batch with an end beyond 1024 bases is filtered on the nibble
    array (ends beyond 448 bases are), and its long reads go to the long launches, which have one build each"""
    bed = beds("rep")
    ctx = filter_ctx(bed, "planes")
    longs = long_pieces(bed.fa, 8)
    reads = bed.reads(0, 100, 300)[:40] + [a for a, _ in longs]
    o_res, o_cig, o_n, _ = bed.expected_se(reads, 0, ("forms-long", 0))
    out = run_se(ctx, reads, 0, "nibbles", 0, stamps, None, f"SE with long reads, stamps {stamps}", long_reads=True)
    compare_se(*out, o_res, o_cig, o_n, reads, "SE with long reads")
    r1, r2 = bed.pairs(0, 100, 200)
    r1, r2 = r1[:20] + [a for a, _ in longs[:4]], r2[:20] + [b for _, b in longs[:4]]
    orc = bed.expected_pe(r1, r2, 0, ("forms-long", 0))
    ctx.set_pe_split(split=1)
    ctx.set_phase_stamps(stamps)
    try:
        gpu = ctx.map_pe(r1, r2, mode=0)
    finally:
        ctx.set_phase_stamps(False)
    got = ctx.last_forms()
    want = expected_pe(True, "nibbles", stamps, None, {}) + [PeForm("whole", True, True, False, False, False, False, False, 1)]
    assert got == want, got
    SEEN.update(got)
    compare_pe(gpu, orc, "pairs with long ends")


@pytest.mark.parametrize("route,flt", [("unsplit", "planes"), ("split", "records")])
def test_trex_forms(oracle, trex_index, workdir, route, flt):
    """the reference's own genome: 300 simulated reads and 200 simulated pairs, on the bit planes and with window records"""
    import abismal_amd as A
    prefix = os.path.join(workdir, "forms_se")
    oracle.simulate(os.path.join(GOLD, "tRex1.fa"), prefix, 300, single_end=True)
    _, reads = ob.read_fastq_like_readloader(prefix + "_1.fq")
    r1, r2 = sim_pairs(oracle, workdir, "forms", n=200)
    oix = oracle.index_load(trex_index)
    try:
        o_res, o_cig, o_n, _ = oracle.map_se(oix, reads, mode=0, threads=8)
        orc = oracle.map_pe(oix, r1, r2, mode=0, threads=8)
    finally:
        oracle.index_free(oix)
    ix = A.Index(trex_index, window_records=172 if flt == "records" else 0)
    ctx = A.Context(ix, 0)
    try:
        assert ctx.filter_on_planes() and ctx.window_records() == (172 if flt == "records" else 0)
        out = run_se(ctx, reads, 0, flt, 2, False, None, "tRex1 SE")
        compare_se(*out, o_res, o_cig, o_n, reads, "tRex1 SE")
        kw = dict(ROUTES)[route]
        ctx.set_pe_split(**kw)
        for text in (None, "sam", "bam"):
            out, _ = run_pe(ctx, r1, r2, 0, flt, kw["split"] != 0, False, text, f"tRex1 PE {route} text {text}")
            compare_pe(out, orc, f"tRex1 PE {route} text {text}")
    finally:
        ctx.close()
        ix.close()


# every build by its fields, as kPeForms / kSeForms list them
def all_builds():
    pe = set()
    for big in (False, True):
        for coop in (True, False):
            pe |= {PeForm("whole", big, False, False, coop, False, False, False, 4), PeForm("whole", big, False, True, coop, False, False, False, 4)}
        pe |= {PeForm("whole", big, False, False, True, False, False, False, 3)}
        pe |= {PeForm("whole", big, False, False, True, False, True, bam, 4) for bam in (False, True)}
        pe |= {PeForm("mate", big, False, timed, False, False, False, False, 4) for timed in (False, True)}
        pe |= {PeForm("mate", big, False, False, False, False, True, bam, 4) for bam in (False, True)}
    pe |= {PeForm("whole", True, False, False, True, True, False, False, 3), PeForm("whole", True, False, False, True, True, False, False, 4),
           PeForm("whole", True, False, True, True, True, False, False, 4), PeForm("whole", True, True, False, False, False, False, False, 1)}
    pe |= {PeForm("seed", False, False, timed, coop, rec, False, False, 4) for timed in (False, True) for coop, rec in ((True, True), (True, False), (False, False))}
    se = {SeForm(timed, coop, rec, bam, False, 5) for coop, rec in ((True, True), (True, False), (False, False))
          for timed, bam in ((False, False), (True, False), (False, True))} | {SeForm(False, False, False, False, True, 1)}
    return pe, se


UNREACHABLE = []  # (forms no batch of this module's scale can reach, each with its reason from the selectors' rules: none)


def test_every_build_ran():
    """the union of the forms the cases above reported is the whole of both tables (it needs them run in the same session)"""
    pe, se = all_builds()
    assert len(pe) == 32 and len(se) == 10 and len(UNREACHABLE) <= 4
    missing = (pe | se) - SEEN - set(UNREACHABLE)
    assert not missing, f"builds no case launched: {sorted(missing, key=str)}"
    assert SEEN <= pe | se, f"forms outside the tables: {sorted(SEEN - (pe | se), key=str)}"
