"""The structures a context derives from the index on the device, entry by entry, and mapping on disordered index files.

Every context builds four things at upload and the mapping kernels then trust them: the genome's bit planes with nmap
(make_planes_kernel), the seed-extension tables (ext_bounds_kernel, ext_gaps_kernel, ext_entries_kernel), the window
records (window_records_kernel) and their hand-over to the launch (build_ext, build_wrec).  Mapping parity cannot see a
table that tabulates nothing ("not tabulated" sends seed_pass down the letter loop, which is exact by construction), a
surplus nmap bit, or a record bit no read's window falls on.  Two things do:

 * tests/hip/index_derived_check.hip (the tests that take `program`): each builder run on its own and every entry compared with
   plain serial host code written from the reference's rules -- letters from the nibble array, std::lower_bound letter by
   letter, the step back when a range empties.  `planes` runs on hand-built genomes; `records` and `tables` on the index
   of synth.repeats_against_n_runs (260 kbp: buckets of 160 copies, entries with blank letters at every depth) as the
   product's own abm_index_build writes it, and `tables` also on two rewritten copies of that file.  The program
   requires its own liveness and prints the counts.
 * the same three files through the C ABI, against the oracle run on the same file (the two `..._on_a_disordered_index_...` tests):
     reversed   every bucket of more than 20 entries, in all three index arrays, has its entries in reverse order
     misplaced  one entry of the 2-letter array swapped with one of a bucket with another key
   with direct narrowing off (narrow_direct relies on the sort and says so; the tables and the letter loop are documented
   not to: DESIGN.md, section 3).

Seeded defects -- each made once in a scratch copy of the tree, the program rebuilt and run on the GPU (on the generator's
default genome; messages abridged).  Each must fail a check here; 1 to 4 are the ones mapping parity cannot see:

 1. ext_entries_kernel writes state 2 for every key: `tables` fails at its first key ("key 2 (base bucket 1): entry lo 0 size
    0 len 0 state 2; the reference's loop gives lo 0 size 18 len 0 state 0").  The library built with it passes
    tests/test_gpu_seed_extension.py and tests/test_gpu_se_parity.py (24 tests) and fails only the comparison this change
    made strict, test_se_tallies_across_index_configurations ("assert 5313462 < 5313462": `<=` held).
 2. the step back on an emptied range is dropped: `tables` fails ("key 19680001 (base bucket 9840000): entry lo 3221 size 0
    len 1 state 0; the reference's loop gives lo 3178 size 43 len 0 state 0").  The library built with it passes the same
    25 tests, the strict comparison included: an emptied range and the range stepped back to (more than maxc entries) both
    yield no candidates.
 3. bnd reads bound[] at a base bucket's boundary instead of the counter: SURVIVES every check (`tables` at maxc 5 and 20
    on the sorted and on the reversed file), and has to: whenever *fail == 0 the two are the same number.  A thread of
    ext_bounds_kernel leaves before filling only on fail or on a descent, and a descent's keys (key < prev) are none; every
    key from 0 to n_keys therefore lies in some thread's gap, and the gap that holds a base bucket's first key b * span
    belongs to the first entry k whose key is >= b * span, which with no entry outside its bucket is counter[b].  A later
    thread of the same bucket fills from its predecessor's key + 1 > b * span on.  With *fail != 0 no table is kept.
 4. the stride of ext_entries_kernel's loop is dropped: `tables` fails at 2-letter + 6 letters ("key 1073741888 (base bucket
    16777217): entry lo 4294967295 size 134217727 len 7 state 3": the program's 0xFF fill, left unwritten); had that key been
    under an empty bucket, the device-side count of non-zero entries would have said so.  Not run as a library against the
    older tests: entries left unwritten are whatever the allocation held, i.e. arbitrary index ranges.  By reading, only
    the 7 + 1 and 2 + 4 letter cases of tests/test_gpu_seed_extension.py build tables beyond 2^30 keys.
 5. `<< (64 - s)` in window_records_kernel becomes `<< (63 - s)`: `records` fails ("record 0 (array 0, entry 0 at 70936),
    bit 58 = base 70911: code 3, expected 1").
 6. `from` in make_planes_kernel ignores kPlaneReach: `planes` fails ("chunk 0 holds a position with a blank within 512
    bases and is not flagged (nmap incomplete)").
 7. p1 is left unwritten: `planes` fails ("block 0 differs between the two copies").

The older suite as a whole was not run against 1 and 2 (12 minutes a run), only the modules named.

Times (MI355X): the compile 12 to 37 s, by the host; `planes` 0.2 s, `records` 0.6 s, `tables` 2.1 s per maxc -- 1.4 s
on the device and comparing, 0.25 s on the host, for all nine configurations (the 2^31-key table and the two of
1.2 x 10^9 included) -- `bigbucket` 0.6 s; each end-to-end test under 4 s.  The bigbucket case fits and is kept."""
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_pe_parity import compare_pe
from tests.test_gpu_se_parity import compare_se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAX_CANDIDATES = (100, 20)
RECORDS = ((0, 0), (100, 108))  # (asked for, serves)
TABLES = ((3, 2), (0, 0))
L = 100
# synth.repeats_against_n_runs with copies at 3-6 % divergence: of the generator's seeds 17 ... 119 at 1-2, 1.5-3, 2-4 and 3-6 %
# none gives every table an entry "finished before its last letter" at every maxc -- the indexer keeps, of each window, the
# position with the smallest letters after it, so the one G->A bucket above 100 entries (the all-purine one) never splits
# within three letters -- and the default (seed 17, 1-2 %) gives the G->A table none at any maxc.  This one misses only
# (G->A, maxc 100): see test_tables_liveness_over_the_three_maxc.
GENOME = dict(seed=34, div=(0.03, 0.06))
LIVE = re.compile(r"(2-letter|C->T|G->A): keys compared (\d+) in \d+ buckets, finished before the last letter (\d+), emptied and stepped back (\d+), still open (\d+)")


# ---- the index file (layout: abismal_amd/csrc/abm_index_file.cpp) and its rewritten copies ---------------------------
def index_arrays(path):
    """the file's bytes, and for each of counter, counter_t, counter_a, index, index_t, index_a its (offset, entries)"""
    raw = np.fromfile(path, dtype=np.uint8)

    def u32(at, n=1):
        return raw[at:at + 4 * n].view("<u4")

    assert bytes(raw[:12]) == b"AbismalIndex"
    at = 12 + 3 * 4
    n_chroms = int(u32(at)[0]); at += 4
    for _ in range(n_chroms):
        at += 4 + int(u32(at)[0])
    starts = u32(at, n_chroms + 1); at += 4 * (n_chroms + 1)
    at += 8 * ((int(starts[-1]) + 15) // 16)  # the genome's nibbles
    at += 4                                   # max_candidates
    counter_size, counter_size3, index_size, index_size3 = (int(x) for x in raw[at:at + 32].view("<u8")); at += 32
    where = {}
    for name, n in (("counter", counter_size + 1), ("counter_t", counter_size3 + 1), ("counter_a", counter_size3 + 1),
                    ("index", index_size), ("index_t", index_size3), ("index_a", index_size3)):
        where[name] = (at, n)
        at += 4 * n
    assert at == len(raw), "index file layout"
    return raw, where


def rewrite(src, dst, change):
    """a copy of the index file `src` whose index arrays went through change(name, counter, index) (in place)"""
    raw, where = index_arrays(src)
    raw = raw.copy()
    for idx_name, cnt_name in (("index", "counter"), ("index_t", "counter_t"), ("index_a", "counter_a")):
        (ia, n), (ca, cn) = where[idx_name], where[cnt_name]
        change(idx_name, raw[ca:ca + 4 * cn].view("<u4"), raw[ia:ia + 4 * n].view("<u4"))
    raw.tofile(dst)


def reverse_big_buckets(name, counter, index, more_than=20):
    sizes = np.diff(counter.astype(np.int64))
    big = np.nonzero(sizes > more_than)[0]
    assert len(big) > 0, f"{name}: no bucket of more than {more_than} entries"
    for b in big:
        lo, hi = int(counter[b]), int(counter[b + 1])
        index[lo:hi] = index[lo:hi][::-1].copy()


def misplace_one(name, counter, index):
    """the 2-letter array only: the first entry of its biggest bucket and the first entry of the next non-empty one (a
    neighbour, so that the keys between two entries stay as few as in the sorted file)"""
    if name != "index":
        return
    sizes = np.diff(counter.astype(np.int64))
    a = int(np.argmax(sizes))
    b = a + 1 + int(np.nonzero(sizes[a + 1:] > 0)[0][0])
    assert sizes[a] > 100
    ia, ib = int(counter[a]), int(counter[b])
    index[ia], index[ib] = int(index[ib]), int(index[ia])


class Bed:
    def __init__(self, oracle, workdir):
        import abismal_amd as A
        self.oracle = oracle
        self.fa = os.path.join(workdir, "index_derived.fa")
        self.lay = synth.repeats_against_n_runs(self.fa, **GENOME)
        self.files = {k: os.path.join(workdir, f"index_derived_{k}.idx") for k in ("sorted", "reversed", "misplaced")}
        A.index_build(self.fa, self.files["sorted"], 4)
        rewrite(self.files["sorted"], self.files["reversed"], reverse_big_buckets)
        rewrite(self.files["sorted"], self.files["misplaced"], misplace_one)
        self._oix, self._se, self._pe, self._ose, self._ope, self._ctx, self._tables_c = {}, {}, None, {}, {}, {}, {}

    def close(self):
        for ix, ctx in self._ctx.values():
            ctx.close()
            ix.close()
        for h in self._oix.values():
            self.oracle.index_free(h)

    def oix(self, which):
        if which not in self._oix:
            self._oix[which] = self.oracle.index_load(self.files[which])
        return self._oix[which]

    def reads(self, mode):
        if mode not in self._se:
            self._se[mode] = synth.trim_like_readloader(synth.reads_against_n_runs(self.lay, self.fa, L, seed=1000 + L, mode=mode))
        return self._se[mode]

    def pairs(self):
        if self._pe is None:
            r1, r2 = synth.pairs_against_n_runs(self.lay, self.fa, L, seed=2000 + L)
            self._pe = (synth.trim_like_readloader(r1), synth.trim_like_readloader(r2))
        return self._pe

    def expected_se(self, which, mode, c):
        """the oracle on the same file; alive: more than 80 % of the reads map and the oracle bisected"""
        if (which, mode, c) not in self._ose:
            reads = self.reads(mode)
            out = self.oracle.map_se(self.oix(which), reads, mode=mode, threads=8, max_candidates=c)
            mapped = float((out[0]["pos"] != 0).sum()) / sum(1 for r in reads if r)
            print(f"SE {which} mode {mode} -c {c}: {len(reads)} reads, oracle maps {mapped:.3f}, {out[3]['search_probes']} probes")
            assert mapped > 0.8 and out[3]["search_probes"] > 0, (which, mode, c, mapped, out[3])
            self._ose[which, mode, c] = out
        return self._ose[which, mode, c]

    def expected_pe(self, which, c):
        if (which, c) not in self._ope:
            r1, r2 = self.pairs()
            out = self.oracle.map_pe(self.oix(which), r1, r2, mode=0, threads=8, max_candidates=c)
            pairs, se1, se2, work = out[0], out[1], out[2], out[5]
            ends = int((pairs["r1"]["pos"] != 0).sum()) * 2 + int(((pairs["r1"]["pos"] == 0) & (se1["pos"] != 0)).sum()) + \
                int(((pairs["r1"]["pos"] == 0) & (se2["pos"] != 0)).sum())
            mapped = ends / float(sum(1 for r in r1 + r2 if r))
            print(f"PE {which} -c {c}: {len(r1)} pairs, oracle maps {mapped:.3f} of the ends, {work['search_probes']} probes")
            assert mapped > 0.8 and work["search_probes"] > 0, (which, c, mapped, work)
            self._ope[which, c] = out
        return self._ope[which, c]

    def ctx(self, which, asked, serves, letters, c):
        """context on file `which` with records asked for `asked` bases and tables of `letters` built for -c `c`; direct
        narrowing off; the tables it ends up with: the letters asked for, or none on the misplaced file"""
        import abismal_amd as A
        key = (which, asked, letters)
        if key not in self._ctx:
            ix = A.Index(self.files[which], seed_extension=letters, window_records=asked)
            ix.set_direct_narrowing(0)
            self._ctx[key] = (ix, A.Context(ix, 0))
            self._tables_c[key] = ix.max_candidates
        ix, ctx = self._ctx[key]
        if letters != (0, 0) and self._tables_c[key] != c:
            ctx.rebuild_seed_extension(c)
            self._tables_c[key] = c
        assert ctx.window_records() == serves, "window records"
        assert ctx.seed_extension()[:2] == ((0, 0) if which == "misplaced" else letters), f"seed-extension tables on the {which} file"
        return ctx


@pytest.fixture(scope="module")
def bed(oracle, workdir):
    b = Bed(oracle, workdir)
    yield b
    b.close()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/hip/index_derived_check.hip, compiled once (narrow_check's command line; it includes abm_kernels.hip and
    abm_ext.hip, not the pair kernels)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("index_derived") / "index_derived_check"
    t0 = time.time()
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "hip", "index_derived_check.hip"), "-o", str(exe)], check=True, timeout=600)
    print(f"index_derived_check compiled in {time.time() - t0:.1f} s")
    return str(exe)


def run_program(program, *args):
    t0 = time.time()
    out = subprocess.run([program, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    print(f"index_derived_check {' '.join(str(a) for a in args[1:])}: {time.time() - t0:.1f} s")
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout


def field(text, name):
    return int(text.split(name + "=")[1].split()[0].rstrip(";"))


@pytest.mark.gpu
def test_planes_nmap_and_iupac_flag(program):
    """plane contents (p0 == p1, code = ctz of the one-hot nibble, 0 for blanks and beyond the genome's words), the IUPAC
    flag (inside n_bases only), nmap complete and tight for every chunk"""
    run_program(program, "-", "planes")


@pytest.mark.gpu
def test_window_records_bit_by_bit(program, bed):
    """records of 3, 4 and 5 blocks over the file's arrays and over positions no index holds: every data bit, the spare
    bits, the record numbering across the three arrays"""
    run_program(program, bed.files["sorted"], "records")


_sorted_runs = {}


def tables_on_the_sorted_file(program, bed, maxc):
    if maxc not in _sorted_runs:
        _sorted_runs[maxc] = run_program(program, bed.files["sorted"], "tables", maxc, "sorted")
    return _sorted_runs[maxc]


@pytest.mark.gpu
@pytest.mark.parametrize("maxc", [5, 20, 100])
def test_tables_key_by_key(program, bed, maxc):
    """every key under a non-empty base bucket against the reference's loop, all other keys counted on the device, both
    gap lists; per table the program requires entries stepped back, entries still open, entries with a blank tabulated
    letter, gaps filled inline and through the list, and that the list of 8 slots overflowed"""
    out = tables_on_the_sorted_file(program, bed, maxc)
    assert field(out, "fail") == 0 and field(out, "fallback_buckets") == 0 and field(out, "overflowed") == 9
    assert len(LIVE.findall(out)) == 3


@pytest.mark.gpu
def test_tables_liveness_over_the_three_maxc(program, bed):
    """entries finished before their last letter: per table, over maxc 5, 20 and 100 together, and for the 2-letter and the
    C->T table at each of them (GENOME's comment: why not for G->A at 100)"""
    early = {}
    for maxc in (5, 20, 100):
        for table, _keys, e, _stepped, _open in LIVE.findall(tables_on_the_sorted_file(program, bed, maxc)):
            early[table, maxc] = int(e)
    print(early)
    for table in ("2-letter", "C->T", "G->A"):
        assert sum(early[table, maxc] for maxc in (5, 20, 100)) > 0, (table, early)
    assert all(early[table, maxc] > 0 for table in ("2-letter", "C->T") for maxc in (5, 20, 100)), early
    assert early["G->A", 5] > 0 and early["G->A", 20] > 0, early


@pytest.mark.gpu
def test_tables_of_reversed_buckets_fall_back(program, bed):
    """buckets out of key order: "not tabulated" for every key under them, everything else as the reference's loop says"""
    out = run_program(program, bed.files["reversed"], "tables", 20)
    assert field(out, "fallback_buckets") > 0 and field(out, "fail") == 0


@pytest.mark.gpu
def test_tables_of_a_misplaced_entry_fail(program, bed):
    """an entry outside the bucket its letters name: *fail is set (2-letter table, every depth); the 3-letter tables of
    the same file are whole"""
    out = run_program(program, bed.files["misplaced"], "tables", 20)
    assert field(out, "fail") == 3


@pytest.mark.gpu
def test_one_bucket_too_big_for_an_entry(program):
    """2^27 + 1 entries in one base bucket (a size does not fit an entry's 27 bits): not tabulated, all else empty"""
    run_program(program, "-", "bigbucket")


def configurations():
    for asked, serves in RECORDS:
        for letters in TABLES:
            for c in MAX_CANDIDATES:
                yield asked, serves, letters, c


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("which", ["reversed", "misplaced"])
def test_se_on_a_disordered_index_equals_the_oracle(bed, which, mode):
    import abismal_amd as A
    reads = bed.reads(mode)
    for asked, serves, letters, c in configurations():
        o_res, o_cig, o_n, _ = bed.expected_se(which, mode, c)
        ctx = bed.ctx(which, asked, serves, letters, c)
        res, cig, off = ctx.map_se(reads, mode=mode, params=A.Params(max_candidates=c))
        compare_se(res, cig, off, o_res, o_cig, o_n, reads, f"SE on the {which} file, mode {mode}, records for {serves}, tables {letters}, -c {c}")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["reversed", "misplaced"])
def test_pe_on_a_disordered_index_equals_the_oracle(bed, which):
    import abismal_amd as A
    r1, r2 = bed.pairs()
    for asked, serves, letters, c in configurations():
        orc = bed.expected_pe(which, c)
        ctx = bed.ctx(which, asked, serves, letters, c)
        compare_pe(ctx.map_pe(r1, r2, mode=0, params=A.Params(max_candidates=c)), orc,
                   f"PE 2 x {L} on the {which} file, records for {serves}, tables {letters}, -c {c}")
