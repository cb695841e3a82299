"""abm_seed_bounds.hpp as plain host C++ under sanitizers: what the sensitive seed pass checks at an offset, from the facts
the specific pass records, against the pass's own conditionals on the counters (tests/cpp/sensitive_bounds_check.cpp)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sensitive_bounds_match_the_counters_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the bounds check"
    exe = tmp_path / "sensitive_bounds_check"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "sensitive_bounds_check.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^(\d+) points, 0 wrong$", r.stdout, re.M)
    # every pair of sizes 0 .. maxc + 2 at both max_candidates, at least once each
    assert m and int(m.group(1)) >= 103 * 103 + 23 * 23, r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
