"""Kernel alone: abm_inflate_bgzf_device over `sim` reads written as BGZF the way bench.py writes it (zlib level 1, blocks
of 0xff00 bytes of text), everything resident in HBM.  GB/s of text at 128, 1,024 and 8,192 blocks per call against what
the mapping kernels consume (README's 22.7 M reads/s times the file's bytes per record).

    python scripts/measure_device_inflate.py [--reads 5000000] [--genome tests/golden/tRex1.fa]   (profiles/device_inflate.log)
"""
import argparse
import os
import subprocess
import sys
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import abismal_amd as A  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=5000000)  # (218 bytes a record: 1.09 GB of text)
ap.add_argument("--genome", default=os.path.join(ROOT, "tests", "golden", "tRex1.fa"))
ap.add_argument("--runs", type=int, default=7)
args = ap.parse_args()
cli = os.path.join(ROOT, "abismal_amd", "abismal-amd")


def member(d):
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    z = co.compress(d) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + (len(z) + 25).to_bytes(2, "little") + z
            + zlib.crc32(d).to_bytes(4, "little") + len(d).to_bytes(4, "little"))


with tempfile.TemporaryDirectory() as wd:
    # (config 2's reads: single-end, 100 bases, the flags bench.py passes)
    subprocess.run([cli, "sim", "-single", "-seed", "1", "-n", str(args.reads), "-l", "100", "-m", "0.01", "-b", "0.98",
                    "-o", os.path.join(wd, "reads"), args.genome], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(wd, "reads_1.fq"), "rb").read()
rec_bytes = len(text) / args.reads
with ThreadPoolExecutor(16) as pool:
    data = b"".join(pool.map(member, [text[k:k + 0xff00] for k in range(0, len(text), 0xff00)]))
blocks, n_text = A.bgzf_scan(data)
assert n_text == len(text)
bar = 22.7e6 * rec_bytes / 1e9
print("%d reads, %.1f bytes a record: %d bytes of text in %d blocks, %d bytes of BGZF (ratio %.2f); the mapping kernels consume %.2f GB/s"
      % (args.reads, rec_bytes, len(text), len(blocks), len(data), len(text) / len(data), bar), flush=True)
dev = torch.device("cuda:0")
d_comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
d_blocks = torch.frombuffer(bytearray(blocks.tobytes()), dtype=torch.uint8).to(dev)
d_text = torch.zeros(n_text, dtype=torch.uint8, device=dev)
d_status = torch.ones(len(blocks), dtype=torch.uint8, device=dev)
with A.Inflater(0) as inf:
    # the whole file once, checked
    inf.inflate_device(d_comp.data_ptr(), len(data), d_blocks.data_ptr(), len(blocks), d_text.data_ptr(), n_text, d_status.data_ptr(), 0)
    torch.cuda.synchronize()
    assert not d_status.cpu().numpy().any() and d_text.cpu().numpy().tobytes() == text
    print("the whole file inflates to the input", flush=True)
    for n in (128, 1024, 8192):
        n = min(n, len(blocks))
        starts = [(k * n) % max(1, len(blocks) - n + 1) for k in range(args.runs)]  # (another part of the file each run)
        ms = []
        for first in starts:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            inf.inflate_device(d_comp.data_ptr(), len(data), d_blocks.data_ptr() + 24 * first, n, d_text.data_ptr(), n_text, d_status.data_ptr(), 0)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        rates = [float(blocks["text_len"][f:f + n].sum()) / 1e9 / (t / 1e3) for f, t in zip(starts, ms)]
        print("%5d blocks a call: ms %s -> GB/s of text %s (the first two: warm-up); median of the rest %.2f = %.2f of %.2f"
              % (n, " ".join("%.3f" % t for t in ms), " ".join("%.2f" % r for r in rates), float(np.median(rates[2:])),
                 float(np.median(rates[2:])) / bar, bar), flush=True)
