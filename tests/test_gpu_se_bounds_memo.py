"""The record-fed single-end kernel's bounds memo (seed_pass; abm_seed_bounds.hpp): the sensitive pass takes the base
buckets of the offsets the specific pass of the same call looked up from LDS instead of the counters.  Results against
the oracle on a genome of 128-copy repeat families (buckets beyond max_candidates), identical twins (exact matches twice:
the specific pass cut short), diverged loci and N runs, at the read lengths where the two passes' offset ranges meet
differently, in every mode (random PBAT: four calls a read, a memo each), with the seed-extension tables at the suite's
default depth, at 4 + 2 letters and absent, and at a max_candidates the tables were not built for (facts from the counters)."""
import os

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_se_parity import compare_se
from tests.test_gpu_se_pilot import GENOME_LEN, family_genome, reads_of

pytestmark = pytest.mark.gpu

# 44, 46: fewer sensitive than specific offsets, ghost bits;  64 / 65;  100: the benchmark's;  128 / 129 / 130: the
# specific pass reaches 64 offsets, then crosses into a second block of them;  172: the longest read the records serve
LENGTHS = (44, 46, 64, 65, 100, 128, 129, 130, 172)
MODES = (0, 1, 2)  # T-rich, A-rich, random PBAT
TABLES = {"default": None, "4,2": (4, 2), "none": (0, 0)}
N_READS = {"family": 150, "twin": 50, "locus": 30, "plain": 40}
N_EXACT = 30
N_RUNS = ((500, 200), (GENOME_LEN // 2 + 137, 40))  # (start, length) of the N runs: before the first slot, and wherever mid-genome (inside a copy, if one lies there)


def exact_reads(seq, places, n, L, rng, mode):
    """n reads that match the genome exactly after conversion, alternately from the forward and the reverse strand, every
    convertible letter converted (C->T; G->A for A-rich reads, for every other read in random PBAT)."""
    out = []
    for k in range(n):
        p, ln = places[int(rng.integers(0, len(places)))]
        at = p + int(rng.integers(0, ln - L + 1))
        s = seq[at:at + L].copy()
        if k & 1:
            s = synth.COMP[s[::-1]]
        a_rich = mode == 1 or (mode == 2 and (k & 2))
        src, dst = (ord("G"), ord("A")) if a_rich else (ord("C"), ord("T"))
        s[s == src] = dst
        out.append(bytes(s).decode())
    return out


class Setup:
    def __init__(self, oracle, workdir):
        import abismal_amd as A
        self.A, self.oracle = A, oracle
        fa = os.path.join(workdir, "bounds_memo.fa")
        self.seq, self.where = family_genome(fa, seed=23)
        for at, n in N_RUNS:
            self.seq[at:at + n] = ord("N")
        with open(fa, "wb") as f:
            f.write(b">chr1\n" + b"\n".join(bytes(self.seq[i:i + 70]) for i in range(0, GENOME_LEN, 70)) + b"\n")
        self.idx = os.path.join(workdir, "bounds_memo.idx")
        A.index_build(fa, self.idx, 8)
        self.oix = oracle.index_load(self.idx)
        self.ctxs, self._reads, self._oracle = {}, {}, {}

    def ctx(self, tables):
        """a context whose launches of these reads are record-fed, with the tables asked for: asserted"""
        if tables not in self.ctxs:
            ix = self.A.Index(self.idx, seed_extension=TABLES[tables], window_records=172)
            ctx = self.A.Context(ix, 0)
            self.ctxs[tables] = (ix, ctx)
            assert ctx.filter_on_planes() and ctx.window_records() == 172, "the launches must be record-fed"
            import abismal_amd.api as api
            want = TABLES[tables] or api.DEFAULT_SEED_EXTENSION
            assert tuple(ctx.seed_extension()[:2]) == tuple(want), "seed-extension tables"
        return self.ctxs[tables][1]

    def reads(self, mode, L):
        if (mode, L) not in self._reads:
            rng = np.random.default_rng(7000 * mode + L)
            pbat = (0.0, 1.0, 0.5)[mode]
            reads = []
            for kind in ("family", "twin", "locus", "plain"):
                reads += reads_of(self.seq, self.where.get(kind), N_READS[kind], L, rng, pbat)
            # around the N runs, and exact matches on either strand (twins: two of them, family copies, anywhere)
            reads += reads_of(self.seq, [(at - L, n + 2 * L + 8) for at, n in N_RUNS], 20, L, rng, pbat)
            reads += exact_reads(self.seq, self.where["twin"] + self.where["family"][:8] + [(5000, 2000)], N_EXACT, L, rng, mode)
            self._reads[mode, L] = synth.trim_like_readloader(reads)  # (the reads that begin or end inside an N run)
        return self._reads[mode, L]

    def expected(self, mode, L, maxc=0):
        key = (mode, L, maxc)
        if key not in self._oracle:
            self._oracle[key] = self.oracle.map_se(self.oix, self.reads(mode, L), mode=mode, threads=8, max_candidates=maxc)[:3]
        return self._oracle[key]

    def close(self):
        for ix, ctx in self.ctxs.values():
            ctx.close()
            ix.close()
        self.oracle.index_free(self.oix)


@pytest.fixture(scope="module")
def memo_setup(oracle, workdir):
    s = Setup(oracle, workdir)
    yield s
    s.close()


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("mode", MODES)
def test_se_bounds_memo_equals_oracle(memo_setup, mode, L):
    s = memo_setup
    reads = s.reads(mode, L)
    o_res, o_cig, o_n = s.expected(mode, L)
    # the fixture does what it is for: reads map (the exact ones at the least; of the 44-base ones with an indel, few), some
    # of them exactly on either strand, some ambiguously
    hit = o_res["pos"] != 0
    exact, rc, ambig = hit & (o_res["diffs"] == 0), (o_res["flags"] & 0x10) != 0, (o_res["flags"] & 0x100) != 0
    print(f"mode {mode} L {L}: {int(hit.sum())} of {len(reads)} mapped, exact {int((exact & ~rc).sum())} + / {int((exact & rc).sum())} -, "
          f"ambiguous {int((hit & ambig).sum())}")
    assert hit.sum() >= N_EXACT and (exact & ~rc).any() and (exact & rc).any() and (hit & ambig).any()
    for tables in TABLES:
        res, cig, off = s.ctx(tables).map_se(reads, mode=mode)
        compare_se(res, cig, off, o_res, o_cig, o_n, reads, f"bounds memo, tables {tables}, mode {mode} L {L}")


@pytest.mark.parametrize("mode,L", [(0, 100), (2, 129), (1, 46)])
def test_se_bounds_memo_facts_from_the_counters(memo_setup, mode, L):
    """max_candidates 20 on tables built for 100: the tables do not apply, the specific pass loads the counters and records
    exact buckets, many of them between 20 and 100 entries."""
    s = memo_setup
    reads = s.reads(mode, L)
    o_res, o_cig, o_n = s.expected(mode, L, maxc=20)
    res, cig, off = s.ctx("default").map_se(reads, mode=mode, params=s.A.Params(max_candidates=20))
    compare_se(res, cig, off, o_res, o_cig, o_n, reads, f"bounds memo at -c 20, mode {mode} L {L}")
