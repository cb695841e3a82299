"""The device FASTQ parser, measured (profiles/device_fastq_parse.log, profiles/device_fastq_parse_ab.log):

(1) the kernels alone: abm_fastq_parse_device over `sim` reads of 100 bases resident in HBM, GB/s of text at 1 MB, about
    7 MB (one slice of 32 k records), 64 MB and 1 GB a call, five calls each, next to one host thread running
    abm_fastq_parse_host on the same text and to the 4.97 GB/s of text the single-end kernels consume;
(2) with --e2e, end to end: `abismal-amd map -gpus 1` over the same reads with ABM_CLI_DEVICE_PARSE=1 and =0 by turns, and
    -- with --parent DIR, a directory holding the parent commit's abismal-amd and libabismal_amd.so -- the parent's map in
    the same session, which shows the off path unchanged.

    python scripts/measure_device_fastq.py [--reads 5000000] [--genome tests/golden/tRex1.fa] [--e2e] [--parent DIR]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import abismal_amd as A  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=5000000)  # (218 bytes a record: 1.09 GB of text)
ap.add_argument("--genome", default=os.path.join(ROOT, "tests", "golden", "tRex1.fa"))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--e2e", action="store_true")
ap.add_argument("--e2e-runs", type=int, default=3)
ap.add_argument("--parent", default=None)
args = ap.parse_args()
cli = os.path.join(ROOT, "abismal_amd", "abismal-amd")
BAR = 4.97  # GB/s of text the single-end kernels consume


def whole_records(newlines, want):
    """the longest prefix of whole records (four lines each) within `want` bytes; newlines: where the text's are"""
    k = int(np.searchsorted(newlines, want, side="left")) // 4  # (records whose last newline lies below `want`)
    return int(newlines[4 * k - 1]) + 1


with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as wd:
    # (config 2's reads: single-end, 100 bases, the flags bench.py passes)
    subprocess.run([cli, "sim", "-single", "-seed", "1", "-n", str(args.reads), "-l", "100", "-m", "0.01", "-b", "0.98",
                    "-o", os.path.join(wd, "reads"), args.genome], check=True, stdout=subprocess.DEVNULL)
    fq = os.path.join(wd, "reads_1.fq")
    text = open(fq, "rb").read()
    print("%d reads, %.1f bytes a record: %d bytes of text; the single-end kernels consume %.2f GB/s of it" % (args.reads, len(text) / args.reads, len(text), BAR),
          flush=True)

    # ---- (1) the kernels alone ---------------------------------------------------------------------------------------------
    lib = A.load_library()
    dev = torch.device("cuda:0")
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    buf = np.frombuffer(text, dtype=np.uint8)
    newlines = np.flatnonzero(buf == 10)
    with A.FastqParser(0) as par:
        for want in (1 << 20, 7 << 20, 64 << 20, 1 << 30):
            n_bytes = whole_records(newlines, want)
            # one host thread first: it also says what the call must give
            info = np.zeros(1, dtype=A.FASTQ_INFO_DTYPE)
            off0 = np.zeros(1, dtype=np.uint64)
            lib.abm_fastq_parse_host(buf.ctypes.data, n_bytes, 44, None, 0, off0.ctypes.data, None, None, 0, info.ctypes.data)
            n, nb = int(info["n_records"][0]), int(info["blob_bytes"][0])
            blob, off = np.zeros(max(1, nb), dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
            name_at, name_len = np.zeros(max(1, n), dtype=np.uint64), np.zeros(max(1, n), dtype=np.uint32)
            host_s = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                rc = lib.abm_fastq_parse_host(buf.ctypes.data, n_bytes, 44, blob.ctypes.data, nb, off.ctypes.data, name_at.ctypes.data, name_len.ctypes.data, n,
                                              info.ctypes.data)
                host_s.append(time.perf_counter() - t0)
                assert rc == 0
            d_blob = torch.zeros(max(1, nb), dtype=torch.uint8, device=dev)
            d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            d_at = torch.zeros(max(1, n), dtype=torch.int64, device=dev)
            d_len = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
            d_info = torch.zeros(A.FASTQ_INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            ms = []
            for _ in range(args.runs + 1):  # (the first call sizes the parser's scratch memory: not counted)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                par.parse_device(d_text.data_ptr(), n_bytes, 44, d_blob.data_ptr(), nb, d_off.data_ptr(), d_at.data_ptr(), d_len.data_ptr(), n, d_info.data_ptr(), 0)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            assert d_info.cpu().numpy().tobytes() == info.tobytes()
            assert d_blob.cpu().numpy()[:nb].tobytes() == blob[:nb].tobytes() and d_off.cpu().numpy().tobytes() == off.tobytes()
            assert d_at.cpu().numpy()[:n].tobytes() == name_at[:n].tobytes() and d_len.cpu().numpy()[:n].tobytes() == name_len[:n].tobytes()
            dev_rates = [n_bytes / 1e9 / (t / 1e3) for t in ms[1:]]
            host_rates = [n_bytes / 1e9 / t for t in host_s]
            print("%10d bytes, %8d records: device ms %s (sizing call %.3f) -> GB/s of text %s, median %.2f = %.2f of %.2f; one host thread GB/s %s, median %.2f; outputs equal"
                  % (n_bytes, n, " ".join("%.3f" % t for t in ms[1:]), ms[0], " ".join("%.2f" % r for r in dev_rates), float(np.median(dev_rates)),
                     float(np.median(dev_rates)) / BAR, BAR, " ".join("%.2f" % r for r in host_rates), float(np.median(host_rates))), flush=True)
            del d_blob, d_off, d_at, d_len
    del d_text
    torch.cuda.empty_cache()

    # ---- (2) end to end ------------------------------------------------------------------------------------------------------
    if args.e2e:
        subprocess.run([cli, "idx", args.genome, os.path.join(wd, "g.idx")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

        def run_map(binary, tag, env):
            tj = os.path.join(wd, "t.json")
            out = os.path.join(wd, tag + ".sam")
            t0 = time.time()
            subprocess.run([binary, "map", "-gpus", "1", "-i", os.path.join(wd, "g.idx"), "-o", out, "-timing", tj, fq],
                           check=True, env=dict(os.environ, **env), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            return json.load(open(tj)), time.time() - t0, out

        variants = [("device", cli, {"ABM_CLI_DEVICE_PARSE": "1"}), ("host", cli, {"ABM_CLI_DEVICE_PARSE": "0"})]
        if args.parent:
            variants.append(("parent", os.path.join(args.parent, "abismal-amd"), {}))
        secs = {v[0]: [] for v in variants}
        for r in range(args.e2e_runs + 1):  # (the first round is warm-up: page cache, code objects)
            for tag, binary, env in variants:
                t, wall, out = run_map(binary, tag, env)
                print("run %d %-6s: %.3f s mapping window, %.3f s wall, %d bytes of SAM, parse %s" % (r, tag, t["seconds"], wall, os.path.getsize(out),
                                                                                                      json.dumps(t.get("parse", {}))), flush=True)
                if r:
                    secs[tag].append(t["seconds"])
        for tag in secs:
            print("%-6s: M reads/s %s" % (tag, " ".join("%.2f" % (args.reads / s / 1e6) for s in secs[tag])), flush=True)
        print("device over host (medians): %.3f" % (float(np.median(secs["host"])) / float(np.median(secs["device"]))), flush=True)
        if args.parent:
            print("host over parent (medians): %.3f" % (float(np.median(secs["parent"])) / float(np.median(secs["host"]))), flush=True)
            print("every host run inside the parent's spread: %s (parent %.3f-%.3f s, host %s)"
                  % (all(min(secs["parent"]) <= s <= max(secs["parent"]) for s in secs["host"]), min(secs["parent"]), max(secs["parent"]),
                     " ".join("%.3f" % s for s in secs["host"])), flush=True)
        print("every device run beats every host run: %s" % (max(secs["device"]) < min(secs["host"])), flush=True)
