"""The carve functions of the mapping kernels (se_carve, pe_carve) against the host-side LDS layouts, on the GPU: a small
HIP program that includes the headers the kernels carve with, built here with hipcc (tests/hip/lds_carve_check.hip)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_every_form_is_carved_where_the_layout_says(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "lds_carve_check"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "hip", "lds_carve_check.hip"), "-o", str(exe)], check=True, timeout=1500)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    # 4 single-end shapes and the long form; 3 pair shapes x (whole, mate) x (small, big) x (plain, text) and seed; the long-end form
    assert out.returncode == 0 and out.stdout.startswith("OK 33 forms"), out.stdout + out.stderr
