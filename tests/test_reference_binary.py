"""CPU: the reference mapper's own `map` and `idx` (oracle/_ref/abismal_ref and abismal_ref_short: its sources compiled
with the stand-in headers of oracle/ref_shims/) against its goldens, and the oracle against what that binary answered on
the edge matrix of tests/reference_edges.py (tests/golden/reference_edges.json).

test_reference_binary_reproduces_the_goldens is what shows that the stand-in SAM writer prints what htslib prints: the
reference's own regression command lines through abismal_ref give the md5s the reference's authors recorded.  Every later
comparison with that binary means something only while this one passes.  The tests that run the binary skip where it is
absent (a machine without the reference tree); the oracle's tests against the manifest never skip."""
import hashlib
import os
import subprocess

import pytest

from tests import reference_edges as E

ROOT = E.ROOT
HAVE_REF = os.path.exists(E.REF) and os.path.exists(E.REF_SHORT)
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/abismal_ref not built (no reference tree on this machine)")
CASES = {c["name"]: c for c in E.CASES}
MAPPED = [c["name"] for c in E.CASES if not c.get("refused")]


def golden():
    return {p: h for h, p in (line.split() for line in open(os.path.join(E.GOLD, "md5sum.txt")))}


@needs_ref
def test_reference_binary_reproduces_the_goldens(oracle, tmp_path_factory):
    """test_scripts/*.test through abismal_ref, reads from the oracle's `sim` (whose FASTQs are md5-pinned too): the index,
    the four SAM files and the four statistics files of data/md5sum.txt."""
    wd = tmp_path_factory.mktemp("ref_chain")
    os.makedirs(wd / "tests")
    os.symlink(os.path.join(E.GOLD, "tRex1.fa"), wd / "tests" / "tRex1.fa")
    sim = ["-seed", "1", "-n", "10000", "-m", "0.01", "-b", "0.98", "tests/tRex1.fa"]
    cmds = [[E.REF, "idx", "tests/tRex1.fa", "tests/tRex1.idx"]]
    for flags, prefix in ((["-single"], "tests/reads"), ([], "tests/reads_pe"), (["-a"], "tests/reads_pbat_pe"), (["-R"], "tests/reads_rpbat_pe")):
        cmds.append([E.ORACLE_CLI, "sim"] + flags + ["-o", prefix] + sim)
    cmds.append([E.REF, "map", "-s", "tests/reads.mstats", "-o", "tests/reads.sam", "-i", "tests/tRex1.idx", "tests/reads_1.fq"])
    for flags, tag in (([], "reads_pe"), (["-P"], "reads_pbat_pe"), (["-P"], "reads_rpbat_pe")):
        cmds.append([E.REF, "map"] + flags + ["-s", f"tests/{tag}.mstats", "-o", f"tests/{tag}.sam", "-i", "tests/tRex1.idx",
                                              f"tests/{tag}_1.fq", f"tests/{tag}_2.fq"])
    for c in cmds:
        r = subprocess.run(c, cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, f"{' '.join(c)}:\n{r.stdout}"
    g = golden()
    assert len(g) == 16
    bad = [p for p, want in g.items() if hashlib.md5(open(wd / p, "rb").read()).hexdigest() != want]
    assert not bad, f"the reference binary's output differs from the reference's goldens: {bad}"


@pytest.fixture(scope="module")
def matrix(oracle, tmp_path_factory):
    """The regenerated inputs, the manifest, every genome's index by the oracle (and by the reference where its binary is
    here), and every `map` run of this module as a job of a small thread pool: the runs are independent processes of a few
    seconds each, so the tests below wait for their own jobs and the module takes a fraction of their sum."""
    from concurrent.futures import ThreadPoolExecutor
    wd = str(tmp_path_factory.mktemp("reference_edges"))
    made = E.make_inputs(wd)
    man = E.load_manifest()
    tools = ["oracle"] + (["ref"] if HAVE_REF else [])
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        built = {(t, n): pool.submit(E.build_index, t, n, wd, os.path.join(wd, f"{t}_{n}.idx")) for t in tools for n in E.INDEXES}
        idx = {k: f.result() for k, f in built.items()}

        def job(tool, case, threads):
            prefix = os.path.join(wd, f"{tool}_{case['name']}_t{threads}")
            extra = ["-t", threads] if tool == "oracle" else []  # (the reference at its default, as it was recorded)
            return E.run_map(tool, case, wd, idx[(tool, case["index"])], prefix, extra=extra), prefix

        jobs = {}
        for tool in tools:
            for case in E.CASES:
                for threads in (["1", "4"] if tool == "oracle" and len(case["reads"]) == 1 and not case.get("refused") else ["1"]):
                    jobs[(tool, case["name"], threads)] = pool.submit(job, tool, case, threads)
        yield {"wd": wd, "made": made, "entries": {e["name"]: e for e in man["cases"]}, "indexes": man["indexes"], "idx": idx, "jobs": jobs}
        for f in jobs.values():
            f.cancel()


def entry_of(matrix, name):
    """the manifest's entry of a case, after checking that it is the case of the table and that its inputs are the recorded ones"""
    case, entry = CASES[name], matrix["entries"].get(name)
    assert entry is not None, f"{name} is not in the manifest: record it (python -m tests.reference_edges --record)"
    assert (entry["index"], entry["flags"], entry["reads"]) == (case["index"], case["flags"], case["reads"]), f"{name}: the manifest records another case"
    assert sorted(entry["inputs"]) == sorted(E.case_inputs(case))
    stale = E.stale_inputs(entry, matrix["made"])
    assert not stale, f"{name}: regenerated inputs differ from the recorded ones: {stale}"
    return case, entry


def test_manifest_covers_the_table(matrix):
    assert sorted(matrix["entries"]) == sorted(CASES) and sorted(matrix["indexes"]) == sorted(E.INDEXES)
    for name in MAPPED:
        assert matrix["entries"][name]["records"] >= CASES[name].get("min_records", E.MIN_RECORDS), name


@pytest.mark.parametrize("index", sorted(E.INDEXES))
def test_oracle_index_is_the_references(matrix, index):
    """byte for byte, window 12 (`-w 12` against the --enable-short build) and `-A targets` included"""
    assert E.md5_file(matrix["idx"][("oracle", index)]) == matrix["indexes"][index], f"oracle idx differs from the reference's for {index}"


def want_of(entry):
    return {k: entry[k] for k in ("records", "sam_md5", "stats_md5")}


@pytest.mark.parametrize("name", MAPPED)
def test_oracle_reproduces_the_reference(matrix, name):
    """the oracle's command line at -t 1, and for single-end input at -t 4 (its shares replay the reads before them, so the
    output is the reference's at -t 1 whatever the thread count), gives the reference's SAM body and statistics"""
    case, entry = entry_of(matrix, name)
    for threads in (["1"] if len(case["reads"]) == 2 else ["1", "4"]):
        r, prefix = matrix["jobs"][("oracle", name, threads)].result()
        assert r.returncode == 0, r.stdout
        got = E.digest(prefix)
        if got != want_of(entry):
            detail = "(no reference binary here to print the records side by side)"
            if HAVE_REF:
                rr, ref_prefix = matrix["jobs"][("ref", name, "1")].result()
                detail = E.first_differences(ref_prefix, prefix, "reference", "oracle") if rr.returncode == 0 else rr.stdout
            pytest.fail(f"{name}, oracle -t {threads}: {got} != recorded {want_of(entry)}\n{detail}")


def test_oracle_refuses_the_read_the_reference_refuses(matrix):
    """32,767 bases: the reference ends with an error status and its "too long" message; so does the oracle's command line"""
    case, entry = entry_of(matrix, "too_long_se")
    assert entry["exit_status"] != 0 and "too long" in entry["message"] and str(E.TOO_LONG) in entry["message"]
    r, _ = matrix["jobs"][("oracle", "too_long_se", "1")].result()
    assert r.returncode != 0 and E.refusal(r.stdout) == entry["message"], r.stdout


@needs_ref
@pytest.mark.parametrize("index", sorted(E.INDEXES))
def test_manifest_indexes_are_current(matrix, index):
    assert E.md5_file(matrix["idx"][("ref", index)]) == matrix["indexes"][index]


@needs_ref
@pytest.mark.parametrize("name", [c["name"] for c in E.CASES])
def test_manifest_is_current(matrix, name):
    """the reference binary still answers what the manifest holds"""
    case, entry = entry_of(matrix, name)
    r, prefix = matrix["jobs"][("ref", name, "1")].result()
    if case.get("refused"):
        assert (r.returncode, E.refusal(r.stdout)) == (entry["exit_status"], entry["message"]), r.stdout
        return
    assert r.returncode == 0, r.stdout
    assert E.digest(prefix) == want_of(entry), f"{name}: the reference answers otherwise: record the manifest again"
