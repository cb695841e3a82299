"""What abm_index_set_iupac_planes buys at scale: kernel milliseconds (abm_ctx_set_timing) of 200 k x 100 bp single-end reads
and 50 k pairs 2 x 150 on the 400 Mbp hg38-shaped genome of tests/test_gpu_scale_parity.py's builder
(bench.synth_genome_fasta) with 50 IUPAC letters scattered in it, for three set-ups, three runs each:

    (i)   the letters, option off     every launch is the nibble build
    (ii)  the letters, option on      planes, records and direct narrowing for all but the chunks around the letters
    (iii) the same genome without the letters

and the ratios (ii)/(iii) and (i)/(ii), with plane_chunks().  Reads neither the oracle nor the reference.

    python scripts/iupac_planes_scale.py [--mbp 400] [--letters 50] [--runs 3] > profiles/iupac_planes_scale.log"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scatter_letters(src, dst, n, seed):
    """a copy of FASTA `src` with n ambiguity letters on bases that are A, C, G or T"""
    raw = np.fromfile(src, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    ok = np.flatnonzero(np.isin(raw, np.frombuffer(b"ACGT", dtype=np.uint8)))
    in_header = np.zeros(len(raw), dtype=bool)
    for at in np.flatnonzero(raw == ord(">")):
        end = at + int(np.argmax(raw[at:] == ord("\n")))
        in_header[at:end] = True
    ok = ok[~in_header[ok]]
    at = rng.choice(ok, n, replace=False)
    raw[at] = np.frombuffer(b"RYMKSWBDHV", dtype=np.uint8)[rng.integers(0, 10, n)]
    raw.tofile(dst)


def host_reads(blob, L):
    return [bytes(r) for r in blob.cpu().numpy().reshape(-1, L)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=400)
    ap.add_argument("--letters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import torch
    import abismal_amd as A
    import bench
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as wd:
        clean_fa, iupac_fa = os.path.join(wd, "clean.fa"), os.path.join(wd, "iupac.fa")
        clean_idx, iupac_idx = os.path.join(wd, "clean.idx"), os.path.join(wd, "iupac.idx")
        bench.synth_genome_fasta(clean_fa, a.mbp, 4321, dev)
        scatter_letters(clean_fa, iupac_fa, a.letters, 5)
        threads = min(16, os.cpu_count() or 8)
        A.index_build(clean_fa, clean_idx, threads)
        A.index_build(iupac_fa, iupac_idx, threads)
        _, starts, gw = bench.read_index_genome(clean_idx)
        se = host_reads(bench.sample_reads(gw, starts, 200_000, 100, 99, dev)[0], 100)
        b1, b2 = bench.sample_pairs(gw, starts, 50_000, 150, 777, dev)
        r1, r2 = host_reads(b1, 150), host_reads(b2, 150)
        setups = (("i: letters, option off", iupac_idx, None), ("ii: letters, option on", iupac_idx, True), ("iii: no letters", clean_idx, None))
        ms = {}
        for label, idx, planes in setups:
            for kind, L in (("se_100", 100), ("pe_150", 150)):
                # (seed-extension tables: none anywhere, so that (ii) and (iii) differ by the letters alone)
                ix = A.Index(idx, seed_extension=(0, 0), window_records=L, iupac_planes=planes)
                ctx = A.Context(ix, 0)
                try:
                    ctx.set_timing(True)
                    run = (lambda: ctx.map_se(se, mode=0)) if kind == "se_100" else (lambda: ctx.map_pe(r1, r2, mode=0))
                    run()  # (warm-up: allocations, code loading)
                    ctx.take_kernel_time()
                    times = []
                    for _ in range(a.runs):
                        run()
                        times.append(ctx.take_kernel_time()[1])
                    ms[label, kind] = times
                    print(f"{label:26s} {kind}: kernel ms {' / '.join(f'{t:.2f}' for t in times)}; filter_on_planes {int(ctx.filter_on_planes())}, "
                          f"records serve {ctx.window_records()}, plane_chunks {ctx.plane_chunks()}", flush=True)
                finally:
                    ctx.close()
                    ix.close()
        for kind in ("se_100", "pe_150"):
            m = {k: statistics.median(ms[label, kind]) for k, (label, _, _) in zip(("i", "ii", "iii"), setups)}
            print(f"{kind}: medians (i) {m['i']:.2f} (ii) {m['ii']:.2f} (iii) {m['iii']:.2f} ms; (ii)/(iii) = {m['ii'] / m['iii']:.4f}, (i)/(ii) = {m['i'] / m['ii']:.3f}")


if __name__ == "__main__":
    main()
