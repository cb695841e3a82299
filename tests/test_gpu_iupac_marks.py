"""The marks a genome with IUPAC letters gets at upload under abm_index_set_iupac_planes, builder by builder.

Mapping parity (tests/test_gpu_iupac_planes.py) cannot see a surplus nmap bit, nor a missing one in a chunk no read of the
fixture starts in, nor a record flag no probe asks.  tests/hip/iupac_marks_check.hip runs make_planes_kernel and
window_records_kernel alone on hand-built genomes -- letters just before, on and just after chunk and block boundaries,
around the reach, on the genome's last base, on the last base a record's stretch covers, on the first past it and 2, 4, 15 and
16 bases past it (the first fifteen lie under the 0xF padding of a window's last word, where a multi-bit nibble lowers
full_compare's sum and so belongs to the record's flag; a blank there, or a letter one base further, does not) -- and
compares nmap chunk by chunk (complete: a marked nibble within kPlaneReach flags the chunk; tight: a flagged chunk has one
within kPlaneReach + 63) and the records' spare bits entry by entry (3, 4 and 5 blocks) with the serial host code of
tests/hip/iupac_marks_host.hpp, with the marking on and off (off: today's arguments, today's outputs -- blanks only).  The host
half builds as plain C++ and prints the counts its fixtures give; test_host_half_counts checks them where there is no GPU.

Seeded defects (all four: tests/test_gpu_iupac_planes.py's docstring).  This program caught the two in the builders: nmap
marks for multi-bit nibbles made without the reach ("chunk 4 holds a position with a marked nibble within 512 bases and is
not flagged (nmap incomplete)") and the record flag set from blanks only ("entry 0 at 8274 has spare bits 0 (low) 0 (high);
its stretch holds a marked nibble or a base past the genome"), and the builder without the margin of 15 bases after the
stretch ("3 blocks: entry 3 at 8083 has spare bits 0 (low) 0 (high)").  Time: the compile 10 s, the run under 1 s."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "tests", "hip")
# what the fixtures of iupac_marks_host.hpp give, by the rules: chunks that must be flagged with the letters marked and
# without, records and how many of them are flagged either way, entries with a letter on their stretch's last covered base
# and on the first base past it
# (by hand, chunks: the first genome's letters flag chunks 1, 2, 4, 5, 7, 8, 10, 11, 15, 16 and its blank chunk 13: 11, 1 with
# the marking off; the three genomes of one letter 2, 3 and 3 against 1 each; the genome of two blanks 3 either way)
COUNTS = ("chunks_must_on=22 chunks_must_off=7 records=1653 records_flagged_on=444 records_flagged_off=69 letter_on_last_covered=84 letter_on_first_past=96 "
          "letter_under_padding=468 letter_just_past_padding=72")


def test_host_half_counts(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "iupac_marks_host")
    subprocess.run([cxx, "-O1", "-std=c++17", os.path.join(HIP, "iupac_marks_host_main.cpp"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip() == "OK host " + COUNTS, out.stdout + out.stderr


@pytest.mark.gpu
def test_nmap_and_record_flags_entry_by_entry(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "iupac_marks_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HIP, "iupac_marks_check.hip"), "-o", exe], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip() == "OK device " + COUNTS, out.stdout + out.stderr
