"""The alignment stages of abm_align.hpp one at a time on the GPU against a serial banded DP: tests/hip/align_check.hip, built
here with hipcc, one sub-command per test; the serial side (tests/hip/align_host.hpp, shared with pilot_score_check.hip) is
checked where there is no GPU, on alignments written out by hand (tests/hip/align_host_main.cpp under ASan and UBSan).

Whole-read parity sees these stages only through reads that happen to map.  Here each runs alone on hand-made input, one
64-lane block per case: table (wavefront<true, false>, wavefront<true, true>, wavefront_rows<true>: every table byte, each
lane's best cell, first_maximum), wrap (reads of 16400 and 20000 bases where the 16-bit narrowing changes score and table),
rounds (score_round<false>, score_round<true>, score_round_quad<false> driven over `first`), floor (score_round_quad<true>),
cigar (cigar_walk + cigar_publish and wave_cigar on every kind of sink; edit_distance and long_enough over a grid), choose
(choose_se<false, false> and choose_se<true, false>).  What each compares, its case sizes and its liveness counts: the
program's header and DESIGN.md section 2.

TIME (MI355X): the six runs take 0.29 - 0.37 s each and `choose`, the slowest, 0.62 s: 2.3 s together.  The program
compiles in 11 s (cross-compiled on the development machine; the module's whole time on the GPU machine, compile included,
was not taken separately: the module passed there as the first of the suite's).

FOUND.  cigar_publish, when a CIGAR of more ops than its slot found no room in the arena, filled the slot from the wrong
end of the walk's ops: the head clip and then the LAST `stride` ops of the CIGAR instead of its first (ctmp[body - 1 - k],
body already cut down to the slot, where ctmp[n - 1 - k] was meant).  `cigar` failed at its first such case ("arena one op
short; L 32, band 27, CIGAR 10M2I9M1D11M, stride 4: slot word expected 160 got 33").  Fixed in abm_align.hpp; the old code
is the last row of the table below.  Also noted, not a defect: the anti-diagonal wavefront<true> leaves cells outside the
read that no step of its schedule falls on unwritten where wavefront_rows<true> writes 3; no walk reads them.  `table`
prefills with 0xEE, accepts that byte from the anti-diagonal runs only in such cells, and counts them (1,777,136).

SEEDED DEFECTS.  Each was built into a copy of the tree and the six sub-commands run against it; the ones that fail:

  defect                                                                      fails
  --------------------------------------------------------------------------  ------------------------------------------
  1  se_window_words one word smaller                                         none -- see below
  1b se_window_words two words smaller                                        table (L 33, band 3: lane 0 best 60 in row 34,
                                                                                  expected 62 in row 35), wrap, rounds, floor, cigar
  2  gs in score_round_quad without the - (K - k) shift                       rounds (score_round_quad<false>, L 33, 7 jobs: a
                                                                                  band-3 job beside a band-61 one scored 4 for
                                                                                  62), floor, choose
  3  wavefront_rows: from-left test against from_prev_lane(c) - 3             table (wavefront_rows<true>, L 33, band 3: row 3
                                                                                  lane 2 expected 1 got 3), cigar, choose
  4  score16 dropped from the from-left candidate of wavefront<TB, true>      none -- see below
  4b score16 dropped from the diagonal candidate instead                      wrap (both lengths)
  5  score_round_quad's fan-out with lanes k + 1 and k + 2 exchanged          rounds (score_round_quad<false>, 5 jobs of band 61:
                                                                                  job 1 scored 46 for 56), floor, choose
  6  cigar_publish: full > arena_cap - at turned into >=                      cigar ("arena fits exactly")
  7  the middle segment's upper bound n_mid1 one iteration later              none -- see below
  7b n_mid1 two iterations later                                              rounds (score_round_quad<false>, L 33, 49 jobs of
                                                                                  band 3: job 4 scored 57 for 55), floor, choose
  8  choose_se's inline rank loop with kk <= key, list_se_jobs left as is     choose (choose_se<false, false>, first set without a
                                                                                  score: ops 3 for 0, flags 0 for ambiguous)
  9  cigar_publish as it was (ctmp[body - 1 - kk])                            cigar ("arena one op short", above)

Every other sub-command passes on each of these builds.  Three defects are NOT caught, and cannot be:
  1   se_window_words keeps a spare word at every length and band: a band's last row needs nibble t0nib + L + bw - 2 of its
      window, at most ((L + bw + 13) >> 4) + 1 words, and the launcher sizes ((L + bw + 30) >> 4) + 1 -- at least one more.
      One word fewer changes nothing the stages read; two fewer (1b) is caught at once.
  4   the from-left candidate is a cell value (0 .. 32767) minus 4, which fits 16 bits as it is: narrowing it is the
      identity, and so is narrowing the from-above candidate.  Only the diagonal candidate can wrap (4b).
  7   in the one extra iteration of the fast path the lane with the largest q computes its q = L - 1 cell without the
      q < L - 1 test of from_above: the cell may take (cell above-right) - 4.  That cell is in the read's last column, so
      nothing descends from it, and the value it may wrongly take is below one the job's best has already seen: no score
      changes.  Two iterations later (7b) a cell past the read is kept.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "tests", "hip")


def test_host_dp_on_written_out_alignments(tmp_path):
    """the serial reference alone, under ASan and UBSan: tables, scores and CIGARs written out in align_host_main.cpp"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "align_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HIP, "align_host_main.cpp"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip() == "OK host 26 tables, 1552 cells, 8 sinks", out.stdout + out.stderr


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("align_check") / "align_check"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HIP, "align_check.hip"), "-o", str(exe)], check=True, timeout=1500)
    return str(exe)


def _run(exe, step):
    out = subprocess.run([exe, step], capture_output=True, text=True, timeout=120)
    print(out.stdout, end="")
    assert out.returncode == 0 and out.stdout.startswith("OK " + step), out.stdout + out.stderr
    return out.stdout


@pytest.mark.gpu
def test_traceback_tables_equal_the_host_table(program):
    _run(program, "table")


@pytest.mark.gpu
def test_sixteen_bit_scores_wrap_as_the_host_dp_does(program):
    _run(program, "wrap")


@pytest.mark.gpu
def test_scoring_rounds_score_every_job_once(program):
    _run(program, "rounds")


@pytest.mark.gpu
def test_rounds_against_a_floor(program):
    _run(program, "floor")


@pytest.mark.gpu
def test_cigar_walk_and_publication_on_every_sink(program):
    _run(program, "cigar")


@pytest.mark.gpu
def test_choose_se_equals_host_choose(program):
    _run(program, "choose")
