"""Single-end alignment in the pilot order (choose_se_pilot: the likeliest job traced first, the others scored against
its score and dropped once beaten) against the oracle, which scores every job to its last row: reads whose candidate
sets hold many alignable entries -- repeat families of 128 copies at 1-30 % divergence (most of them at the low end,
where seeds still find them), identical twins, loci with a gap-free but more diverged copy -- with and without a short
indel in mid-read.  Result tests: they hold for any order of the work; only the tally check at the end is about the
mechanism."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_se_parity import compare_se

pytestmark = pytest.mark.gpu

GENOME_LEN = 300_000
FAM_LEN, FAM_COPIES, N_FAMS = 400, 128, 3
TWIN_LEN, N_TWINS = 300, 12
LOCUS_LEN, N_LOCI = 300, 12
N_READS = {"family": 1400, "twin": 400, "locus": 400, "plain": 300}


def family_genome(path, seed=11):
    """One chromosome of random sequence with, at disjoint places: N_FAMS families of FAM_COPIES copies whose divergence
    from the family's consensus rises from 1 % to 30 % (as the eighth power of the copy number; substitutions only),
    N_TWINS segments present twice, letter for letter, and N_LOCI loci with a second copy 8 % diverged, substitutions
    only.  Returns where each kind lies."""
    rng = np.random.default_rng(seed)
    seq = synth.ACGT[rng.integers(0, 4, GENOME_LEN)].copy()
    slots = rng.permutation(np.arange(1000, GENOME_LEN - 1000, 500))  # disjoint 500-base slots
    take = iter(slots.tolist())
    where = {"family": [], "twin": [], "locus": []}

    def diverged(piece, div):
        out = piece.copy()
        m = rng.random(len(piece)) < div
        out[m] = synth.ACGT[(np.searchsorted(synth.ACGT, out[m]) + rng.integers(1, 4, int(m.sum()))) % 4]
        return out

    for _ in range(N_FAMS):
        fam = synth.ACGT[rng.integers(0, 4, FAM_LEN)]
        for k in range(FAM_COPIES):
            at = next(take)
            seq[at:at + FAM_LEN] = diverged(fam, 0.01 + 0.29 * (k / (FAM_COPIES - 1)) ** 8)
            where["family"].append((at, FAM_LEN))
    for _ in range(N_TWINS):
        a, b = next(take), next(take)
        seq[b:b + TWIN_LEN] = seq[a:a + TWIN_LEN]
        where["twin"] += [(a, TWIN_LEN), (b, TWIN_LEN)]
    for _ in range(N_LOCI):
        a, b = next(take), next(take)
        seq[b:b + LOCUS_LEN] = diverged(seq[a:a + LOCUS_LEN], 0.08)
        where["locus"].append((a, LOCUS_LEN))
    with open(path, "wb") as f:
        f.write(b">chr1\n" + b"\n".join(bytes(seq[i:i + 70]) for i in range(0, GENOME_LEN, 70)) + b"\n")
    return seq, where


def reads_of(seq, places, n, L, rng, pbat_frac):
    """n reads of L bases from the given (start, length) places (None: anywhere): either strand, one or two
    substitutions, in three reads of ten an insertion or deletion of 1-3 bases in mid-read, bisulfite-converted."""
    out = []
    for _ in range(n):
        if places is None:
            at = int(rng.integers(0, GENOME_LEN - L - 8))
        else:
            p, ln = places[int(rng.integers(0, len(places)))]
            at = p + int(rng.integers(0, ln - L - 8 + 1))
        frag = seq[at:at + L + 8].copy()
        if rng.random() < 0.5:
            frag = synth.COMP[frag[::-1]]
        s = frag
        if rng.random() < 0.3:
            k, mid = int(rng.integers(1, 4)), L // 2 + int(rng.integers(-5, 6))
            if rng.random() < 0.5:
                s = np.concatenate([frag[:mid], synth.ACGT[rng.integers(0, 4, k)], frag[mid:]])
            else:
                s = np.concatenate([frag[:mid], frag[mid + k:]])
        s = s[:L].copy()
        for j in rng.integers(0, L, int(rng.integers(1, 3))):
            s[j] = synth.ACGT[(int(np.searchsorted(synth.ACGT, s[j])) + int(rng.integers(1, 4))) % 4]
        src, dst = (ord("G"), ord("A")) if rng.random() < pbat_frac else (ord("C"), ord("T"))
        conv = (s == src) & (rng.random(L) < 0.95)
        s[conv] = dst
        out.append(bytes(s).decode())
    return out


@pytest.fixture(scope="module")
def family_setup(oracle, workdir):
    import abismal_amd as A
    fa = os.path.join(workdir, "families.fa")
    seq, where = family_genome(fa)
    idx = os.path.join(workdir, "families.idx")
    A.index_build(fa, idx, 8)
    ix = A.Index(idx)
    ctx = A.Context(ix, 0)
    oix = oracle.index_load(idx)
    yield seq, where, ctx, oix
    oracle.index_free(oix)
    ctx.close()
    ix.close()


@pytest.mark.parametrize("mode,L", [(0, 50), (0, 100), (0, 150), (2, 50), (2, 100), (2, 150)])
def test_se_pilot_order_equals_oracle(oracle, family_setup, mode, L):
    seq, where, ctx, oix = family_setup
    rng = np.random.default_rng(1000 * mode + L)
    pbat = 0.5 if mode == 2 else 0.0
    reads = []
    for kind in ("family", "twin", "locus", "plain"):
        reads += reads_of(seq, where.get(kind), N_READS[kind], L, rng, pbat)
    # the fixture does what it is for: a family read's set holds more jobs than one scoring round takes
    n_family = N_READS["family"]
    _, _, _, fam_work = oracle.map_se(oix, reads[:n_family], mode=mode, threads=8)
    print(f"mode {mode} L {L}: {fam_work['aligns'] / n_family:.1f} alignments per family read")
    assert fam_work["aligns"] > 12 * n_family
    o_res, o_cig, o_cig_n, _ = oracle.map_se(oix, reads, mode=mode, threads=8)
    res, cig, cig_off = ctx.map_se(reads, mode=mode)
    compare_se(res, cig, cig_off, o_res, o_cig, o_cig_n, reads, f"families mode {mode} L {L}")
    assert int((res["pos"] != 0).sum()) > 0.5 * len(reads)


def test_pilot_order_equals_host_dp(tmp_path):
    """tests/hip/pilot_score_check.hip: choose_se in the pilot order against a plain host DP that scores every job, on
    3000 built job sets (see the program's head for what they contain)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "pilot_score_check"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "hip", "pilot_score_check.hip"), "-o", str(exe)], check=True, timeout=1500)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def test_scoring_rounds_end_early(family_setup):
    """The diagnostic build's tally: on the family reads the scoring rounds run fewer iterations than rounds that go
    to their last rows would, i.e. the floor is engaged -- and the results above are the oracle's all the same."""
    seq, where, ctx, _ = family_setup
    reads = reads_of(seq, where["family"], N_READS["family"], 100, np.random.default_rng(5), 0.0)
    ctx.take_work()
    ctx.set_phase_stamps(True)
    try:
        ctx.map_se(reads, mode=0)
        work = ctx.take_work()
    finally:
        ctx.set_phase_stamps(False)
    ran, full = work["score_iterations"], work["score_iterations_full"]
    print(f"scoring iterations: {ran} run, {full} in full ({ran / max(1, full):.3f})")
    assert 0 < ran < full
