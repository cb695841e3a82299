"""Stage 3 of seed_pass (abm_seed.hpp) -- the Hamming filter -- routine by routine on the GPU against a plain letter-by-letter
count: tests/hip/filter_check.hip, built here with hipcc, one sub-command per test; the serial side
(tests/hip/filter_host.hpp) is checked where there is no GPU, on cases written out by hand (tests/hip/filter_host_main.cpp
under ASan and UBSan).

Whole-read parity sees the filter only through the best one or two distances of a read.  Here every routine runs alone, one
wave per workgroup and one case per workgroup, on planes and records built by the product's own kernels and in LDS carved by
se_carve: masks (build_qmasks, q_window16), distance (hamming_planes_pairs, hamming_planes<1 / 2 / 4> with groups of four and
eight lanes, hamming_records_lane<false / true>, both overloads of hamming, hamming2), step (filter_step_windows<true / false>,
filter_step_records<SeSet>, every field of every FilterStep, with a model of the position cache), replay (replay_chunk on
SeSet against libstdc++'s heap calls; the pair set's appending path), ghost (ghost_bits against a simulation of the
reference's reused buffers).  What each compares, the cases and the liveness counts: the program's header and DESIGN.md
section 2.  Every comparison is exact.

TIME (MI355X, as each sub-command reports it): masks 0.3 - 0.4 s, ghost 0.2 - 0.3 s, replay 0.2 - 0.3 s, step 0.3 s, distance
1.5 s (1.2 s of it the host building a genome of 145 M bases with every planted copy; 12,790 cases and 1.5 M distances in the
other 0.4 s): under 3 s together.  The program compiles in 30 - 34 s.

FOUND: no defect in abm_seed.hpp; no kernel code changed.  Two things the work made explicit.  (1) The position cache's
contents after a step are not a function of the candidates alone: two different positions that lanes of one half write to one
slot leave either of them there (one LDS store instruction, no specified winner).  Distances are unaffected (a hit is exact by
construction); only FilterStep::cached and the loads saved depend on it.  The model keeps the set of possible contents and
accepts hit_lo .. hit_hi for such a lookup.  So that this cannot quietly become "anything goes", `step` requires the lookups
held to a hit to outnumber the open ones four to one (13,069 against 1,219 and 4,907 against 440), and a third of the window
cases with 65 candidates or more draw their positions from a pool in which no two share a slot: there the model must be sure
of every lookup (the program fails if it is not) and `cached` is compared with one number, hits and slot collisions included
(exact_cases, exact_cache_hits, exact_slot_collisions).  (2) An empty slot is the value 0, so the entry's position must be
compared in full -- see defect 8.

SEEDED DEFECTS.  Each was built into a copy of the tree and the five sub-commands run against it on the MI355X; the ones that fail:

  defect                                                                   fails
  -----------------------------------------------------------------------  ---------------------------------------------
  1  hamming_planes: b1 = b0 + 2 for G == 4                                distance (hamming_planes<2>, L 130, G 4, lane 5 a half,
                                                                               shift 63, planted change at 0: expected 1 got 2), step
                                                                               (filter_step_windows<true>, L 150: h expected 95 got 96)
  2  hamming_planes: `counts` with <=                                      distance (hamming_planes<2>, L 64, G 4, slot 16 alone wanted:
                                                                               expected 1 got 45), step (L 192, G 4: h 133 got 161)
  3  group_sum without the row_half_mirror step                            distance (hamming_planes<2>, L 257, G 8, planted change at
                                                                               256: expected 1 got 0), step (L 300, G 8: h 208 got 176)
  4  hamming_planes_pairs: skip test shifted by pass * 32                  none, with today's code generation -- see below
  5  hamming2: c - 1 < nwords turned into c < nwords                       distance (hamming2, L 128 = 8 words, planted change at 112:
                                                                               expected d 1 dmax 1, got d 0 dmax 0)
  6  hamming_records_lane: qm for the second block                         distance (hamming_records_lane<false>, L 65, exact copy,
                                                                               record 8993, x 83: expected 0 got 40), step
                                                                               (filter_step_records, L 100: offered expected 1 got 0)
  7  build_qmasks: past-the-end nibble 0                                   masks (L 35, encoding 0, block 0, code 0, base 35: mask bit 0,
                                                                               expected 1), distance (hamming_planes_pairs, L 35:
                                                                               expected 1 got 30), step (L 50, G 2: h 32 got 46)
  8  PosCacheEntry::matches on the low 24 bits                             step (filter_step_windows<true>, first candidate of a call at
                                                                               pos 16777216: h expected 32 got 0) -- and nothing else can
  9  filter_step_records: || fa removed from ca                            step (filter_step_records, IUPAC genome, L 50, cutoff 20:
                                                                               offered (a flagged record) expected 1 got 0)
  10 replay_chunk: no re-mask after the cutoff fell                        replay (case 0, uniform distances, L 60: wt.updates expected
                                                                               91 got 95)
  11 replay_chunk: first ballot on h                                       replay (case 0: wt.updates expected 91 got 100)
  12 ghost_bits: lt >= k                                                   ghost (batch 0, read 3 of 39 bases, encoding 2, word 0:
                                                                               first differing position 39)

Every other sub-command passes on each of these builds.
  4   changes nothing a caller can see in the code this compiler generates today -- the row rests on that, not on the
      language.  The test reads (second ? wb : wa) >> ((pass & 1) * 32); with pass * 32 the amount is
      64 and 96 in passes 2 and 3.  The loop is `#pragma unroll 1`, so pass is a run-time value and the shift is one 64-bit
      shift instruction, which takes its amount modulo 64: 64 -> 0 and 96 -> 32, the very amounts of (pass & 1) * 32.  As C++
      the shift is undefined, and a compiler that unrolled the loop could fold it to anything -- to a test of the wrong
      32 slots, for one.  That outcome WOULD be caught: `distance` wants single slots in every quarter (0, 15, 16, 31 | 32, 63 |
      64, 95 | 96, 127), so a pass skipped for the wrong quarter leaves a wanted slot without its distance.  The build as it
      stands skips exactly the passes it skipped before: all 3,882 skipped passes of `distance` and every want pattern give
      the same distances.
  8   is caught through one door only.  Two different positions that share a slot always differ in their low 24 bits: the
      slot is the top byte of pos * 0x9E3779B1, and adding k << 24 to pos moves that byte by 0xB1 * k mod 256, which is not 0
      for k = 1 .. 255 (0xB1 is odd).  So among written entries 24 bits decide as 32 do.  An EMPTY slot (0) is what differs:
      it then "holds" every position whose low 24 bits are 0, with distances 0 / 0.  `step` proposes windows at 2^24 for
      that reason, some of them before anything else has used their slot (a genome of 2^24 + 16 k bases); mapping parity
      would need a read whose best hit lies exactly there.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "tests", "hip")


def test_host_side_on_written_out_cases(tmp_path):
    """the serial side alone, under ASan and UBSan: distances, cache, set and ghost letters written out in filter_host_main.cpp"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "filter_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HIP, "filter_host_main.cpp"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip() == "OK host 82 checks", out.stdout + out.stderr


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("filter_check") / "filter_check"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HIP, "filter_check.hip"), "-o", str(exe)], check=True, timeout=1500)
    return str(exe)


def _run(exe, step, live):
    """run one sub-command; every liveness count named in `live` must be in the OK line and above zero"""
    out = subprocess.run([exe, step], capture_output=True, text=True, timeout=150)
    print(out.stdout, end="")
    assert out.returncode == 0 and out.stdout.startswith("OK " + step), out.stdout + out.stderr
    counts = {}
    section = ""
    for word in out.stdout.split():
        if word.endswith(":"):
            section = word[:-1]
        m = re.fullmatch(r"([A-Za-z0-9_^]+)=(\d+);?", word)
        if m:
            counts.setdefault(m.group(1), []).append((section, int(m.group(2))))
    for name, times in live.items():
        got = counts.get(name, [])
        assert len(got) == times, f"{step}: liveness count {name} printed {len(got)} times, expected {times}: {out.stdout}"
        for section, value in got:
            assert value > 0, f"{step}: liveness count {name} ({section}) is zero: {out.stdout}"
    return out.stdout


@pytest.mark.gpu
def test_masks_and_read_windows(program):
    out = _run(program, "masks", {"mask_bits": 1, "past_end_bits": 1, "untouched_words": 1, "windows": 1})
    m = re.search(r"nibbles 0/1/2/4/5/8/10=([\d/]+);", out)
    assert m and all(int(x) > 0 for x in m.group(1).split("/")), out


@pytest.mark.gpu
def test_each_distance_routine_alone(program):
    _run(program, "distance", {"compared": 1, "copy1_windows": 1, "passes_skipped": 1, "last_block_windows": 1, "dmax_gt_d": 1,
                               "last_record": 1, "one_half_cases": 1, "slots_not_wanted": 1, "exact_copies": 1, "one_off_copies": 1})


@pytest.mark.gpu
def test_filter_steps_as_seed_pass_drives_them(program):
    _run(program, "step", {"cache_hits": 2, "slot_collisions": 2, "exact_cases": 2, "exact_cache_hits": 2, "exact_slot_collisions": 2, "redone": 3, "twice_in_step": 1, "at_2^24": 1, "steps_with_b": 3,
                           "steps_without_b": 3, "offered": 1, "dropped_by_cutoff": 1, "flagged_kept": 1, "unflagged_dropped": 1})


@pytest.mark.gpu
def test_replay_chunk_against_the_heap_calls(program):
    _run(program, "replay", {"updates": 1, "fifo_updates": 1, "invalid_lanes_between_valid": 1, "hmax_above_h_below_cutoff": 1,
                             "refused_after_mid_chunk_tightening": 1, "chunks_cut_by_sure_ambig": 1, "exact_hits": 1,
                             "sensitive_calls": 1, "full_sets": 1, "pair_set_appended": 1, "pair_set_hmax_refused": 1})


@pytest.mark.gpu
def test_ghost_bits_against_the_reused_buffers(program):
    _run(program, "ghost", {"words_compared": 1, "letters_from_donors": 1, "donor_1_back": 1, "donor_64_back": 1, "donor_65_back": 1,
                            "donor_150_back": 1, "zero_fill_letters": 1, "of_them_at_or_past_max_len": 1, "reads_without_donor": 1,
                            "reads_with_several_donors": 1, "short_reads_between": 1})
