"""The pair kernels' steps between a finished candidate set and a mated pair (PeWave, abm_pe_wave.hpp), one at a time on
the GPU against serial host code: tests/hip/pe_mate_check.hip, built here with hipcc, one sub-command per test.

Whole-pair parity with the oracle (test_gpu_pe_parity.py, test_gpu_pe_full_sets.py) sees these steps only through the
pair that comes out at the end; an entry or two wrong at a window's far edge, or a word written past a table whose
neighbour happens to be rewritten in time, pass there.  Here each step runs alone on hand-made lists -- freeze
(heap_order_now / freeze_heap_order), sort (sort_unique: radix passes, both bitonic networks), search (sample_list /
search_list), marks (mark_pairable), scan (scan_pairs) -- in the tier-1, tier-2 and (sort, search) long-end forms.  What
each compares with, its case sizes and its liveness counts: the program's header and DESIGN.md section 2.

SEEDED DEFECTS.  Each of these was built into a copy of the tree and this module run against it; the tests that fail:

  defect                                                                     fails
  -------------------------------------------------------------------------  ---------------------------------------
  sample_list with the shift it had before (first s with n >> s <= 512)      search: 513 samples at n = 1,025, one of the 16
                                                                                 words behind samp overwritten
  one sample in fifty 300 bases too high at samp_shift >= 5                  search: 10 samples differ from the list at
                                                                                 n = 16,384 (and the searches behind them)
  the radix scatter gives a digit's lanes one slot too few, lists > 20,000   sort: 303 positions left of 20,001
  the shift == 24 pass skipped (its digit taken as 0)                        sort: first list of 513 full-range positions
  STRICT ignored in the hi search of scan_pairs                              scan: tier 1, lists of 5 and 70, limits 150..300
  lane 0's `seen` taken as 0 instead of prev_hi                              scan: tier 1, lists of 5 and 70: the kept scr1
  carry not propagated across chunks (list index clamped to the list)        scan: tier 1, lists of 5 and 70, limits 32..40,000

Every other test passes on each of these builds -- marks and scan, which search through the same samples, on the two
sample builds as well: only `search` pins the samples.  The sixth was NOT caught by the first version of `scan`: the pair a call
records last -- the one whose scores it hands on -- fell on lane 0 of a later group of 64 list-1 entries in none of 936
calls.  Score table 4 (list 1's scores rising, each group's first entry above the rest) puts it there: 30 tier-1 and 6
tier-2 calls, counted and required by the program.

The defect test_gpu_pe_full_sets.py records as passing the whole suite is the second row.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "hip", "pe_mate_check.hip")


def _build(exe, *defines):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), *defines, SOURCE,
                    "-o", str(exe)], check=True, timeout=1500)
    return str(exe)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pe_mate_check") / "pe_mate_check")


@pytest.fixture(scope="module")
def bitonic_program(tmp_path_factory):
    """the same program with the radix sort's threshold out of reach: tier 2 sorts every list by its bitonic network"""
    return _build(tmp_path_factory.mktemp("pe_mate_check_bitonic") / "pe_mate_check", "-DABM_PE_RADIX_SORT_MIN=1000000")


def _run(exe, step):
    out = subprocess.run([exe, step], capture_output=True, text=True, timeout=120)
    print(out.stdout, end="")
    assert out.returncode == 0 and out.stdout.startswith("OK " + step), out.stdout + out.stderr
    return out.stdout


@pytest.mark.gpu
def test_lists_frozen_in_libstdcxx_heap_order(program):
    _run(program, "freeze")


@pytest.mark.gpu
def test_sort_unique_equals_std_sort_and_full_compare(program):
    assert "beyond 512 entries by radix passes" in _run(program, "sort")


@pytest.mark.gpu
def test_sort_unique_by_the_bitonic_network_alone(bitonic_program):
    assert "beyond 1000000 entries by radix passes" in _run(bitonic_program, "sort")


@pytest.mark.gpu
def test_sampled_search_equals_std_bounds_and_stays_inside_its_table(program):
    _run(program, "search")


@pytest.mark.gpu
def test_pairable_marks_equal_brute_force(program):
    _run(program, "marks")


@pytest.mark.gpu
def test_scan_pairs_equals_best_pair_loops(program):
    _run(program, "scan")
