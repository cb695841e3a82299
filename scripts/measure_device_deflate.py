"""Device BGZF deflate, measured (profiles/device_bgzf_deflate_ab.log):

(1) the kernels alone: abm_deflate_bgzf_device (deflate_bgzf_kernel + pack_bgzf_kernel) over a real `map -B` record stream
    resident in HBM, GB/s of text at 128, 1,024 and 8,192 blocks of 0xff00 bytes a call, and inflate_bgzf_kernel
    (abm_inflate_bgzf_device) over the very members the deflater wrote, for comparison;
(2) end to end: `abismal-amd map -B` over the same reads with ABM_CLI_DEVICE_DEFLATE=1 and =0 by turns, and -- with
    --parent DIR, a directory holding the parent commit's abismal-amd and libabismal_amd.so -- the parent's map -B in the
    same session, which shows the off path unchanged.

    python scripts/measure_device_deflate.py [--reads 5000000] [--genome tests/golden/tRex1.fa] [--parent DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import abismal_amd as A  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=5000000)
ap.add_argument("--genome", default=os.path.join(ROOT, "tests", "golden", "tRex1.fa"))
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--e2e-runs", type=int, default=3)
ap.add_argument("--parent", default=None)
args = ap.parse_args()
cli = os.path.join(ROOT, "abismal_amd", "abismal-amd")
BLOCK = 0xff00


def stored_bam_text(path):
    """the record stream of a BAM written at -z 0"""
    raw, out, at = open(path, "rb").read(), [], 0
    while at < len(raw):
        n = int.from_bytes(raw[at + 16:at + 18], "little") + 1
        out.append(zlib.decompress(raw[at + 18:at + n - 8], -15))
        at += n
    return b"".join(out)


def timed(call, runs):
    ms = []
    for k in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(k)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def report(what, n, ms, text_bytes):
    rates = [t_b / 1e9 / (t / 1e3) for t_b, t in zip(text_bytes, ms)]
    print("%-8s %5d blocks a call: ms %s -> GB/s of text %s (the first two: warm-up); median of the rest %.2f"
          % (what, n, " ".join("%.3f" % t for t in ms), " ".join("%.2f" % r for r in rates), float(np.median(rates[2:]))), flush=True)


with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as wd:
    # (config 2's reads: single-end, 100 bases, the flags bench.py passes)
    subprocess.run([cli, "idx", args.genome, os.path.join(wd, "g.idx")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.run([cli, "sim", "-single", "-seed", "1", "-n", str(args.reads), "-l", "100", "-m", "0.01", "-b", "0.98",
                    "-o", os.path.join(wd, "reads"), args.genome], check=True, stdout=subprocess.DEVNULL)
    fq = os.path.join(wd, "reads_1.fq")

    def run_map(binary, tag, env, flags=()):
        tj = os.path.join(wd, "t.json")
        out = os.path.join(wd, tag + ".bam")
        t0 = time.time()
        subprocess.run([binary, "map", "-gpus", "1", "-B"] + list(flags) + ["-i", os.path.join(wd, "g.idx"), "-o", out, "-timing", tj, fq],
                       check=True, env=dict(os.environ, **env), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        t = json.load(open(tj))
        return t, time.time() - t0, out

    # ---- (1) the kernels alone -------------------------------------------------------------------------------------------
    _, _, stored = run_map(cli, "stored", {}, ["-z", "0"])
    text = stored_bam_text(stored)
    n_blocks = -(-len(text) // BLOCK)
    print("%d reads mapped -B: %d bytes of BAM records (%.1f a read) = %d blocks of 0xff00" % (args.reads, len(text), len(text) / args.reads, n_blocks), flush=True)
    dev = torch.device("cuda:0")
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_out = torch.zeros(A.bgzf_deflate_bound(len(text)), dtype=torch.uint8, device=dev)
    d_blocks = torch.zeros(n_blocks * 24, dtype=torch.uint8, device=dev)
    d_total = torch.zeros(1, dtype=torch.int64, device=dev)
    with A.Deflater(0) as de, A.Inflater(0) as inf:
        # the first 1,024 blocks once, against the host's bytes; then the whole text once, inflated again on the device
        n_chk = min(1024, n_blocks) * BLOCK
        de.deflate_device(d_text.data_ptr(), min(n_chk, len(text)), 0, d_out.data_ptr(), d_out.numel(), d_total.data_ptr(), d_blocks.data_ptr(), 0)
        torch.cuda.synchronize()
        want, _ = A.deflate_bgzf_host(text[:n_chk])
        assert d_out[:int(d_total.item())].cpu().numpy().tobytes() == want
        print("the device's members of the first %d blocks are the host encoder's, byte for byte" % min(1024, n_blocks), flush=True)
        de.deflate_device(d_text.data_ptr(), len(text), 0, d_out.data_ptr(), d_out.numel(), d_total.data_ptr(), d_blocks.data_ptr(), 0)
        torch.cuda.synchronize()
        total = int(d_total.item())
        blocks = np.frombuffer(d_blocks.cpu().numpy().tobytes(), dtype=A.BGZF_BLOCK_DTYPE).copy()
        d_back = torch.zeros(len(text), dtype=torch.uint8, device=dev)
        d_status = torch.ones(n_blocks, dtype=torch.uint8, device=dev)
        inf.inflate_device(d_out.data_ptr(), total, d_blocks.data_ptr(), n_blocks, d_back.data_ptr(), len(text), d_status.data_ptr(), 0)
        torch.cuda.synchronize()
        assert not d_status.cpu().numpy().any() and bool(torch.equal(d_back, d_text))
        print("the whole text: %d bytes of BGZF (ratio %.2f), inflated on the device to the input" % (total, len(text) / total), flush=True)
        d_members = d_out.clone()  # (the timed deflate calls below write d_out)
        d_desc = d_blocks.clone()
        for n in (128, 1024, 8192):
            n = min(n, n_blocks)
            starts = [(k * n) % max(1, n_blocks - n + 1) for k in range(args.runs)]  # (another part of the text each run)
            sizes = [min(len(text), (f + n) * BLOCK) - f * BLOCK for f in starts]
            ms = timed(lambda k: de.deflate_device(d_text.data_ptr() + starts[k] * BLOCK, sizes[k], 0, d_out.data_ptr(), d_out.numel(),
                                                   d_total.data_ptr(), d_blocks.data_ptr(), 0), args.runs)
            report("deflate", n, ms, sizes)
            ms = timed(lambda k: inf.inflate_device(d_members.data_ptr(), total, d_desc.data_ptr() + 24 * starts[k], n, d_back.data_ptr(), len(text),
                                                    d_status.data_ptr(), 0), args.runs)
            report("inflate", n, ms, sizes)
    del d_text, d_out, d_back, d_members
    torch.cuda.empty_cache()

    # ---- (2) end to end ----------------------------------------------------------------------------------------------------
    variants = [("device", cli, {"ABM_CLI_DEVICE_DEFLATE": "1"}), ("host", cli, {"ABM_CLI_DEVICE_DEFLATE": "0"})]
    if args.parent:
        variants.append(("parent", os.path.join(args.parent, "abismal-amd"), {}))
    secs = {v[0]: [] for v in variants}
    for r in range(args.e2e_runs + 1):  # (the first round is warm-up: page cache, code objects)
        for tag, binary, env in variants:
            t, wall, out = run_map(binary, tag, env)
            how = t.get("deflate", {})
            print("run %d %-6s: %.3f s mapping window, %.3f s wall, %d bytes of BAM, deflate %s" % (r, tag, t["seconds"], wall, os.path.getsize(out), json.dumps(how)), flush=True)
            if r:
                secs[tag].append(t["seconds"])
    for tag in secs:
        print("%-6s: M reads/s %s" % (tag, " ".join("%.2f" % (args.reads / s / 1e6) for s in secs[tag])), flush=True)
    print("device over host (medians): %.3f" % (float(np.median(secs["host"])) / float(np.median(secs["device"]))), flush=True)
    if args.parent:
        print("host over parent (medians): %.3f" % (float(np.median(secs["parent"])) / float(np.median(secs["host"]))), flush=True)
    print("every device run beats every host run: %s" % (max(secs["device"]) < min(secs["host"])), flush=True)
