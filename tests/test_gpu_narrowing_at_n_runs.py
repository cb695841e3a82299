"""Bucket narrowing where the probed genome letters lie in an N run.

Every narrowing path of the kernels reads genome letters from a structure that cannot say N -- the pair kernels'
narrow_both<REC> from the window records, narrow_direct from the bit planes, the seed-extension tables from whatever the
letter loop they tabulate reads -- and each has a way back to the nibble array: record_nibble where a record's N flag is set
(or the probe is beyond the record's reach), narrow_direct's `ok = false` after which seed_pass runs the letter loop.  The
reference orders and bisects a blank nibble as 2-letter bit 1 and 3-letter symbol 0; the planes and records hold code 0
(= A) there, which is bit 0 and, in the C->T alphabet, symbol 1.

Two things reach those ways back:

 * tests/hip/narrow_check.hip (test_narrowing_functions_against_lower_bound): the three functions themselves, thousands
   of cases on a hand-built index whose ranges hold entries with blank letters from every depth 25 ... 255, against
   std::lower_bound on the nibble array;
 * synth.repeats_against_n_runs (everything else here): a repeat family with copies cut short by long N runs, so that
   buckets of more than max_candidates entries hold entries whose letters at depth 25 and more are blank, mapped through
   the C ABI in every combination of window records, seed-extension tables, direct-narrowing threshold and -c, single-end
   and paired, against the oracle bit for bit.  The fixture's liveness -- the ORACLE's bisections probed blank nibbles on
   both kinds of table -- is asserted on the CPU (test_fixture_probes_blank_letters), before any GPU visit.

Which builds these catch -- each tried once on a copy of the tree, every configuration below run on its own:

 1. record_nibble ignores the records' N flag: narrow_check fails (narrow_both<true>, first at a 2-letter range of 331
    entries).  End to end it fails the pairs of 2 x 100 at -c 20 wherever the index has records (for 108 and for 172 bases;
    every mode, table depth, direct-narrowing threshold and launch form; 5 of 360 pairs differ) and passes everything else:
    single-end and pairs without records read no records, and at -c 100 and at 2 x 150 no misplaced boundary changes a
    pair's result on this fixture -- the oracle probes blank letters there (test_fixture_probes_blank_letters), the pairs
    are found through their other seeds.
 2. window_records_kernel never sets the flag: narrow_check fails at once (the records' flags are compared with the nibble
    array entry by entry); end to end exactly the cases of 1.
 3. seed_pass takes narrow_direct's result whatever `ok` says: when this was tried narrow_check restated seed_pass's rule,
    so the change made to seed_pass alone did not reach it; made to the restated rule as well, narrow_check failed at its
    first case.  (It now runs the kernel's own narrow_direct_chains, abm_seed.hpp, which is where such a change would be
    made.)  End to end the change to seed_pass fails 114 of the 144 single-end configurations and 108 of
    the 144 paired-end ones in which the threshold is 16 or 64, every launch form (whose threshold is the default, 64), and
    none with direct narrowing off."""
import os
import shutil
import subprocess
import time

import pytest

from tests import synth
from tests.test_gpu_pe_filter_paths import alive
from tests.test_gpu_pe_parity import compare_pe
from tests.test_gpu_pe_split import FORMS
from tests.test_gpu_se_parity import compare_se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENGTHS = (100, 150)
MODES = (0, 1, 2)
MAX_CANDIDATES = (100, 20)
RECORDS = ((0, 0), (100, 108), (172, 172))  # (asked for, serves)
TABLES = ((0, 0), (3, 2))
DIRECT_FROM = (0, 16, 64)


class NRunBed:
    """the genome, its index, the reads and pairs cut from it, the oracle's results (once per input, mode and -c) and one
    context per (window records, seed-extension letters)"""

    def __init__(self, oracle, workdir):
        self.oracle = oracle
        self.fa = os.path.join(workdir, "repeats_against_n_runs.fa")
        self.idx = os.path.join(workdir, "repeats_against_n_runs.idx")
        self.lay = synth.repeats_against_n_runs(self.fa)
        oracle.index_build(self.fa, self.idx, threads=4)
        self.oix = oracle.index_load(self.idx)
        self._se, self._pe, self._ose, self._ope, self._ctx, self._tables_c = {}, {}, {}, {}, {}, {}

    def close(self):
        for ix, ctx in self._ctx.values():
            ctx.close()
            ix.close()
        self.oracle.index_free(self.oix)

    def reads(self, L, mode):
        if (L, mode) not in self._se:
            self._se[L, mode] = synth.trim_like_readloader(synth.reads_against_n_runs(self.lay, self.fa, L, seed=1000 + L, mode=mode))
        return self._se[L, mode]

    def pairs(self, L, mode):
        """mode 1 (PBAT): the A-rich end comes first; mode 2 (random PBAT): in every other pair"""
        if (L, mode) not in self._pe:
            r1, r2 = synth.pairs_against_n_runs(self.lay, self.fa, L, seed=2000 + L)
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
            self._ose[L, mode, c] = self.oracle.map_se(self.oix, self.reads(L, mode), mode=mode, threads=8, max_candidates=c)
        return self._ose[L, mode, c]

    def expected_pe(self, L, mode, c):
        if (L, mode, c) not in self._ope:
            r1, r2 = self.pairs(L, mode)
            self._ope[L, mode, c] = self.oracle.map_pe(self.oix, r1, r2, mode=mode, threads=8, max_candidates=c)
        return self._ope[L, mode, c]

    def ctx(self, asked, serves, letters, c):
        """the context with window records asked for `asked` bases and seed-extension tables of `letters`, its tables built
        for -c `c` (a table answers only for the max_candidates it was built with), its path asserted"""
        import abismal_amd as A
        key = (asked, letters)
        if key not in self._ctx:
            ix = A.Index(self.idx, seed_extension=letters, window_records=asked)
            self._ctx[key] = (ix, A.Context(ix, 0))
            self._tables_c[key] = ix.max_candidates
        ix, ctx = self._ctx[key]
        if letters != (0, 0) and self._tables_c[key] != c:
            ctx.rebuild_seed_extension(c)
            self._tables_c[key] = c
        assert ctx.window_records() == serves, "window records"
        assert ctx.filter_on_planes(), "the filter must run on the bit planes"
        assert ctx.seed_extension()[:2] == letters, "seed-extension tables"
        return ix, ctx


@pytest.fixture(scope="module")
def bed(oracle, workdir):
    b = NRunBed(oracle, workdir)
    yield b
    b.close()


def test_fixture_probes_blank_letters(bed):
    """Liveness of the fixture, on the oracle alone (no GPU): for every read length, mode and -c the GPU tests use, the
    oracle's bisections probed blank nibbles on the 2-letter table and on the 3-letter ones, narrowed at all, and mapped
    more than 80 % of the reads and pairs; and every paired input has a pair with fallback hits only."""
    for L in LENGTHS:
        for mode in MODES:
            for c in MAX_CANDIDATES:
                res, _, _, work = bed.expected_se(L, mode, c)
                reads = bed.reads(L, mode)
                mapped = float((res["pos"] != 0).sum()) / sum(1 for r in reads if r)
                print(f"SE L {L} mode {mode} -c {c}: {len(reads)} reads, {mapped:.3f} mapped, {work['search_probes']} probes, "
                      f"blank letters probed: {work['blank_probes2']} (2-letter), {work['blank_probes3']} (3-letter)")
                assert work["blank_probes2"] > 0 and work["blank_probes3"] > 0, (L, mode, c, work)
                assert work["search_probes"] > 0
                assert mapped > 0.8, (L, mode, c, mapped)
                orc = bed.expected_pe(L, mode, c)
                work = orc[5]
                print(f"PE 2 x {L} mode {mode} -c {c}: blank letters probed: {work['blank_probes2']} (2-letter), "
                      f"{work['blank_probes3']} (3-letter)")
                alive(orc, f"PE 2 x {L} mode {mode} -c {c}")
                assert work["blank_probes2"] > 0 and work["blank_probes3"] > 0, (L, mode, c, work)


def configurations():
    for asked, serves in RECORDS:
        for letters in TABLES:
            for c in MAX_CANDIDATES:
                yield asked, serves, letters, c


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("mode", MODES)
def test_se_across_every_narrowing_path(bed, mode, L):
    """single-end: window records for 0 / 108 / 172 bases, no tables and 3 + 2 letters, direct narrowing from 0 (never) /
    16 / 64 entries, -c 100 and 20"""
    import abismal_amd as A
    reads = bed.reads(L, mode)
    for asked, serves, letters, c in configurations():
        o_res, o_cig, o_n, _ = bed.expected_se(L, mode, c)
        ix, ctx = bed.ctx(asked, serves, letters, c)
        for direct in DIRECT_FROM:
            ix.set_direct_narrowing(direct)
            res, cig, off = ctx.map_se(reads, mode=mode, params=A.Params(max_candidates=c))
            compare_se(res, cig, off, o_res, o_cig, o_n, reads,
                       f"SE L {L} mode {mode}, records for {serves}, tables {letters}, direct narrowing from {direct}, -c {c}")


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("mode", MODES)
def test_pe_across_every_narrowing_path(bed, mode, L):
    """paired-end, the same grid: with records that serve L the record-fed seed kernel narrows with letters from the
    records (record_nibble), otherwise from the nibble array; ranges from the threshold on go through narrow_direct"""
    import abismal_amd as A
    r1, r2 = bed.pairs(L, mode)
    for asked, serves, letters, c in configurations():
        orc = bed.expected_pe(L, mode, c)
        ix, ctx = bed.ctx(asked, serves, letters, c)
        for direct in DIRECT_FROM:
            ix.set_direct_narrowing(direct)
            compare_pe(ctx.map_pe(r1, r2, mode=mode, params=A.Params(max_candidates=c)), orc,
                       f"PE 2 x {L} mode {mode}, records for {serves}, tables {letters}, direct narrowing from {direct}, -c {c}")


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("mode", MODES)
def test_pe_record_fed_across_launch_forms(bed, mode, L):
    """the record-fed seed kernel in every launch form of tests/test_gpu_pe_split.py (one kernel per pair, seed / mate split
    with lists in LDS, in the staging area, with a hand-over area that runs out), at -c 100 and 20"""
    import abismal_amd as A
    r1, r2 = bed.pairs(L, mode)
    ix = A.Index(bed.idx, seed_extension=(0, 0), window_records=172)
    ctx = A.Context(ix, 0)
    try:
        assert ctx.window_records() == 172 and ctx.filter_on_planes() and ctx.seed_extension()[:2] == (0, 0)
        for form, kw in FORMS:
            ctx.set_pe_split(**kw)
            for c in MAX_CANDIDATES:
                compare_pe(ctx.map_pe(r1, r2, mode=mode, params=A.Params(max_candidates=c)), bed.expected_pe(L, mode, c),
                           f"PE 2 x {L} mode {mode}, records for 172, {form}, -c {c}")
    finally:
        ctx.close()
        ix.close()


@pytest.mark.gpu
def test_narrowing_functions_against_lower_bound(tmp_path):
    """tests/hip/narrow_check.hip: narrow_both<false>, narrow_both<true> and narrow_direct + seed_pass's use of it against
    std::lower_bound on the nibble array; the program asserts its own liveness (blank letters probed, `ok` both ways, flagged
    records probed, per table) and prints the counts."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "narrow_check"
    # (the compile takes 50-55 s on one host thread: the program includes abm_kernels.hip for launch_make_planes, and abm_ext.hip,
    # but not the pair kernels; the run itself takes about a second)
    t0 = time.time()
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "hip", "narrow_check.hip"), "-o", str(exe)], check=True, timeout=600)
    print(f"narrow_check compiled in {time.time() - t0:.1f} s")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
