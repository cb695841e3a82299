"""GPU: the product's command line against what the reference mapper itself answered on the edge matrix of
tests/reference_edges.py -- recorded in tests/golden/reference_edges.json from the reference's own sources, with no oracle in
between.  `abismal-amd idx` must write the reference's index file byte for byte (window 12 and `-A targets` included) and
`abismal-amd map <flags>` the reference's SAM body (all but the @PG line) and statistics file, once as a plain run and once
cut into tiny slices with the SAM text written on the device.  Inputs are regenerated here; one whose md5 is not the
recorded one fails the case by name.  Only when an md5 differs is the oracle run, to tell the reader which of the two
restatements of the reference -- the kernels or the oracle -- is off."""
import os

import pytest

from tests import reference_edges as E

pytestmark = pytest.mark.gpu
CASES = {c["name"]: c for c in E.CASES}
MAPPED = [c["name"] for c in E.CASES if not c.get("refused")]
# tiny slices, batches of 3000 and device-written SAM text, as in tests/test_gpu_cli_goldens.py
TINY = dict(ABM_CLI_SLICE_READS="997", ABM_CLI_DEVICE_SAM="1", ABM_CLI_BATCH_READS="3000")


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    """the regenerated inputs, the manifest and one index per genome, built by the product's indexer"""
    wd = str(tmp_path_factory.mktemp("gpu_reference_edges"))
    made = E.make_inputs(wd)
    man = E.load_manifest()
    idx = {name: E.build_index("product", name, wd, os.path.join(wd, f"product_{name}.idx"), timeout=300) for name in E.INDEXES}
    return {"wd": wd, "made": made, "entries": {e["name"]: e for e in man["cases"]}, "indexes": man["indexes"], "idx": idx, "oracle_idx": {}}


def entry_of(matrix, name):
    case, entry = CASES[name], matrix["entries"].get(name)
    assert entry is not None, f"{name} is not in the manifest"
    assert (entry["index"], entry["flags"], entry["reads"]) == (case["index"], case["flags"], case["reads"]), f"{name}: the manifest records another case"
    stale = E.stale_inputs(entry, matrix["made"])
    assert not stale, f"{name}: regenerated inputs differ from the recorded ones: {stale}"
    return case, entry


@pytest.mark.parametrize("index", sorted(E.INDEXES))
def test_index_file_is_the_references(matrix, index):
    assert E.md5_file(matrix["idx"][index]) == matrix["indexes"][index], f"abismal-amd idx differs from the reference's index for {index}"


def product_map(matrix, case, prefix, env):
    """One `abismal-amd map` run.  A run that is killed by a signal or by its time limit ends the session: nothing more is
    started on a GPU that a process has just died on."""
    import subprocess
    try:
        r = E.run_map("product", case, matrix["wd"], matrix["idx"][case["index"]], prefix, env=env, timeout=180)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"abismal-amd map hung on {case['name']}: {e}", returncode=3)
    if r.returncode < 0 or r.returncode >= 128:
        pytest.exit(f"abismal-amd map died on {case['name']} (status {r.returncode}):\n{r.stdout}", returncode=3)
    return r


def blame(matrix, case, entry, product_prefix):
    """the oracle on the same inputs: does it give the recorded answer, and where does the product leave it"""
    wd, name = matrix["wd"], case["index"]
    if name not in matrix["oracle_idx"]:
        matrix["oracle_idx"][name] = E.build_index("oracle", name, wd, os.path.join(wd, f"oracle_{name}.idx"))
    prefix = os.path.join(wd, "oracle_" + case["name"])
    r = E.run_map("oracle", case, wd, matrix["oracle_idx"][name], prefix, extra=["-t", "4"] if len(case["reads"]) == 1 else [])
    if r.returncode != 0:
        return "the oracle failed on these inputs:\n" + r.stdout
    same = E.digest(prefix) == {k: entry[k] for k in ("records", "sam_md5", "stats_md5")}
    verdict = ("the oracle gives the recorded answer: the product is off" if same else
               "the oracle does not give the recorded answer either: the restatement the kernels were written to is off")
    return verdict + "\n" + E.first_differences(prefix, product_prefix, "oracle", "product")


@pytest.mark.parametrize("units", ["defaults", "tiny_slices_device_sam"])
@pytest.mark.parametrize("name", MAPPED)
def test_map_reproduces_the_reference(matrix, oracle, name, units):
    """When this matrix was first run, the twelve cases whose input is se.fq or holds it missed 1 to 7 records each
    (se_default 1772 of 1775): reads that the reference's reader trims below the minimum length after counting their letters,
    which the reference maps and the kernels skipped (test_reads_that_trimming_left_below_the_minimum_length)."""
    case, entry = entry_of(matrix, name)
    env = dict(os.environ, **TINY) if units != "defaults" else None
    prefix = os.path.join(matrix["wd"], f"product_{name}_{units}")
    r = product_map(matrix, case, prefix, env)
    assert r.returncode == 0, r.stdout
    got, want = E.digest(prefix), {k: entry[k] for k in ("records", "sam_md5", "stats_md5")}
    print(f"{name} [{units}]: {got}")
    if got != want:
        pytest.fail(f"{name} [{units}]: {got} != recorded {want}\n{blame(matrix, case, entry, prefix)}")


def test_a_read_of_32767_bases_is_refused(matrix):
    """The reference takes reads of up to 32,766 bases.  On one of 32,767 its reader throws "found a read of size 32767,
    which is too long. Maximum allowed read size = 32767" inside a worker thread, so the run dies on the uncaught exception
    (status -6 recorded) with the SAM cut off after its header.  The product's command line refuses the same input while
    it parses it, with the same message and an ordinary error status; the library underneath, given such a read directly,
    hands it back unmapped and counts it (abm_ctx_reads_too_long, include/abismal_amd.h: test_reads_beyond_16383_bases)."""
    case, entry = entry_of(matrix, "too_long_se")
    assert entry["exit_status"] != 0 and "too long" in entry["message"]
    for env in (None, dict(os.environ, **TINY)):
        r = product_map(matrix, case, os.path.join(matrix["wd"], "product_too_long"), env)
        assert r.returncode == 1, r.stdout
        assert E.refusal(r.stdout) == entry["message"], r.stdout


@pytest.mark.parametrize("window", [20, 12])
def test_reads_that_trimming_left_below_the_minimum_length(oracle, tmp_path, window):
    """What the matrix found, through the C ABI and read by read: the reference's reader asks for key weight + window - 1
    letters other than N BEFORE it trims (src/abismal.cpp:187-195), so a read that began with IUPAC letters reaches the
    mapper shorter than that, and is mapped (only an exact match can be reported, :308-313).  Reads of every length from
    the shortest the library maps (35 bases with window 20, 29 with window 12) to 3 beyond the minimum, exact copies and
    copies with one substitution, either strand, among ordinary reads so that their seeds past the end see earlier reads'
    letters: hits, flags and CIGARs equal the oracle's, single-end (T-rich and random PBAT) and as ends of pairs, and the
    exact copies below the minimum do map.  One base shorter than that is left unmapped."""
    import numpy as np
    import abismal_amd as A
    from tests import synth
    from tests.test_gpu_pe_parity import compare_pe
    from tests.test_gpu_se_parity import compare_se
    fa = os.path.join(E.GOLD, "tRex1.fa")
    idx = str(tmp_path / "t.idx")
    oracle.index_build(fa, idx, threads=4, window=window)
    lo, min_len = (35, 44) if window == 20 else (29, 36)
    chroms = synth.read_chroms(fa)
    rng = np.random.default_rng(window)
    reads, mates, short_exact = [], [], []
    for k in range(600):
        ch = chroms[k % 2]
        L = 100 if k % 3 == 0 else int(rng.integers(lo, min_len + 3))
        at = int(rng.integers(1000, len(ch) - 1000))
        frag = ch[at:at + 300].copy()
        s = frag[:L].copy()
        if k % 3 == 2:
            s[int(rng.integers(0, L))] = synth.ACGT[rng.integers(0, 4)]
        elif L < min_len:
            short_exact.append(k)
        m = synth.COMP[frag[::-1]][:100].copy()
        if k % 2:
            s, m = synth.COMP[s[::-1]], synth.COMP[m[::-1]]
        reads.append(bytes(s).decode().replace("C", "T").replace("N", "A"))
        mates.append(bytes(m).decode().replace("G", "A").replace("N", "T"))
    ix = A.Index(idx)
    ctx = A.Context(ix, 0)
    oix = oracle.index_load(idx)
    try:
        for mode in (0, 2):
            res, cig, off = ctx.map_se(reads, mode=mode)
            o_res, o_cig, o_n, _ = oracle.map_se(oix, reads, mode=mode, threads=1)
            compare_se(res, cig, off, o_res, o_cig, o_n, reads, f"reads of {lo}-{min_len + 2} bases, window {window}, mode {mode}")
        assert len(short_exact) > 50 and sum(int(o_res["pos"][k]) != 0 for k in short_exact) > len(short_exact) // 2
        compare_pe(ctx.map_pe(reads, mates, mode=2), oracle.map_pe(oix, reads, mates, mode=2, threads=1), f"ends of {lo}-{min_len + 2} bases, window {window}")
        res, _, _ = ctx.map_se([reads[0], reads[short_exact[0]][:lo - 1], reads[0]])
        assert int(res["pos"][1]) == 0 and int(res["pos"][0]) == int(res["pos"][2]) != 0
    finally:
        oracle.index_free(oix)
        ctx.close()
        ix.close()
