"""Text deflated into BGZF blocks on the GPU (abm_deflate_bgzf, abm_deflate_bgzf_device, `map -B` with
ABM_CLI_DEVICE_DEFLATE=1, `bgzf -device`): byte for byte what abm_deflate_bgzf_host -- the same encoder run serially on the
CPU, checked against zlib in tests/test_bgzf_deflate_host.py -- makes of the same text."""
import ctypes as C
import gzip
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import abismal_amd as A
from tests import bam_format as B
from tests import deflate_cases as K
from tests import deflate_tools as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "abismal_amd", "abismal-amd")
CANARY = 4096
LIMIT = 300  # seconds a child process may take (it takes a few)


@pytest.fixture(scope="module")
def deflater():
    d = A.Deflater(0)
    yield d
    d.close()


# ---- bytes ---------------------------------------------------------------------------------------------------------------
def test_every_case_gives_the_hosts_bytes(deflater):
    # texts shorter than one hash (0 .. 3 bytes), one round of 64 and one either side of it, matches that cross a round's
    # end, a match that ends on the block's last byte, a block of exactly 0xff00, the stored fallback (random, high), a
    # distance of exactly 32768 and of 32769
    for i, data, bb in K.every_text() + K.window_edge_texts():
        want, want_blocks = A.deflate_bgzf_host(data, bb)
        got, blocks = deflater.deflate(data, bb)
        assert got == want, i
        assert K.blocks_equal(blocks, want_blocks), i


def run_raw(deflater, data, block_bytes, out_cap):
    """abm_deflate_bgzf into a buffer with canaries either side: (rc, buffer, *out_bytes, blocks)"""
    lib = A.load_library()
    buf = np.frombuffer(data, dtype=np.uint8)
    n_cap = -(-len(buf) // (block_bytes or K.BLOCK))
    out = np.full(out_cap + 2 * CANARY, 0xC5, dtype=np.uint8)
    blocks = np.zeros(n_cap, dtype=A.BGZF_BLOCK_DTYPE)
    n_out, n_blocks = C.c_uint64(), C.c_uint64()
    rc = lib.abm_deflate_bgzf(deflater.handle, buf.ctypes.data, len(buf), block_bytes, out.ctypes.data + CANARY, out_cap, C.byref(n_out),
                              blocks.ctypes.data, n_cap, C.byref(n_blocks))
    assert n_blocks.value == n_cap
    return rc, out, n_out.value, blocks


@pytest.fixture(scope="module")
def many_blocks():
    """1,500 blocks of 7919 bytes with the host's encoding: a megabyte of the BAM-like stream and one of FASTQ text, over
    and over (7919 is prime, so every block begins somewhere else in them)"""
    text = ((K.bam_stream(1000000) + D.fastq_text(1000000)) * 6)[:1500 * 7919]
    assert len(text) == 1500 * 7919
    return text, A.deflate_bgzf_host(text, 7919)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1500])
def test_block_counts(deflater, many_blocks, n):
    text, (want, want_blocks) = many_blocks
    end = int(want_blocks[n - 1]["at"]) + int(want_blocks[n - 1]["len"])
    cap = A.bgzf_deflate_bound(n * 7919, 7919)
    rc, out, n_out, blocks = run_raw(deflater, text[:n * 7919], 7919, cap)
    assert rc == 0 and n_out == end
    assert out[CANARY:CANARY + end].tobytes() == want[:end] and K.blocks_equal(blocks, want_blocks[:n])
    assert (out[:CANARY] == 0xC5).all() and (out[CANARY + end:] == 0xC5).all()  # nothing but [0, out_bytes) is touched


def test_a_capacity_one_short_is_reported_and_nothing_is_written(deflater, many_blocks):
    text, (want, want_blocks) = many_blocks
    end = int(want_blocks[63]["at"]) + int(want_blocks[63]["len"])
    rc, out, n_out, blocks = run_raw(deflater, text[:64 * 7919], 7919, end - 1)
    assert rc == A.ERR_CAPACITY and n_out == end
    assert (out == 0xC5).all() and not blocks["len"].any()


def test_two_deflaters_from_two_threads(many_blocks):
    text, (want, want_blocks) = many_blocks
    out = [None, None]

    def work(k):
        d = A.Deflater(0)
        try:
            out[k] = d.deflate(text, 7919)
        finally:
            d.close()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for got, blocks in out:
        assert got == want and K.blocks_equal(blocks, want_blocks)


def test_device_entry_point_on_a_torch_stream(deflater, many_blocks):
    import torch
    text, (want, want_blocks) = many_blocks
    n = 200
    text = text[:n * 7919]
    end = int(want_blocks[n - 1]["at"]) + int(want_blocks[n - 1]["len"])
    dev = torch.device("cuda:0")
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_out = torch.full((end + 2 * CANARY,), 0xC5, dtype=torch.uint8, device=dev)
    d_blocks = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
    d_total = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        deflater.deflate_device(d_text.data_ptr(), len(text), 7919, d_out.data_ptr() + CANARY, end, d_total.data_ptr(), d_blocks.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    got = d_out.cpu().numpy()
    assert int(d_total.item()) == end
    assert got[CANARY:CANARY + end].tobytes() == want[:end]
    assert (got[:CANARY] == 0xC5).all() and (got[CANARY + end:] == 0xC5).all()
    assert K.blocks_equal(np.frombuffer(d_blocks.cpu().numpy().tobytes(), dtype=A.BGZF_BLOCK_DTYPE), want_blocks[:n])
    # a capacity one byte short: the total still says what is needed, and nothing at or beyond the capacity is written
    d_out.fill_(0xC5)
    d_total.zero_()
    deflater.deflate_device(d_text.data_ptr(), len(text), 7919, d_out.data_ptr() + CANARY, end - 1, d_total.data_ptr(), d_blocks.data_ptr(), 0)
    torch.cuda.synchronize(dev)
    got = d_out.cpu().numpy()
    assert int(d_total.item()) == end
    assert got[CANARY:CANARY + end - 1].tobytes() == want[:end - 1]
    assert (got[:CANARY] == 0xC5).all() and (got[CANARY + end - 1:] == 0xC5).all()
    # no text: no member
    d_total.fill_(77)
    deflater.deflate_device(0, 0, 0, 0, 0, d_total.data_ptr(), 0, 0)
    torch.cuda.synchronize(dev)
    assert int(d_total.item()) == 0


def test_round_trip_on_the_device(deflater, many_blocks):
    text, _ = many_blocks
    text = text[:300 * 7919] + K.cases()["high"][:70000] + K.cases()["zeros"][:70000]
    out, blocks = deflater.deflate(text)
    scanned, n_text = A.bgzf_scan(out)
    assert n_text == len(text) and K.blocks_equal(scanned, blocks)
    with A.Inflater(0) as inf:
        back, status = inf.inflate(out, scanned, n_text)
    assert not status.any() and back == text


# ---- through the CLI ---------------------------------------------------------------------------------------------------
def test_cli_bgzf_on_the_device(tmp_path):
    data = K.bam_stream(300000) + K.cases()["random"][:70000] + D.fastq_text(100000)
    (tmp_path / "in.bin").write_bytes(data)
    subprocess.run([CLI, "bgzf", "-device", "0", str(tmp_path / "in.bin"), str(tmp_path / "out.gz")], check=True, timeout=LIMIT)
    raw = (tmp_path / "out.gz").read_bytes()
    assert gzip.open(tmp_path / "out.gz").read() == data
    assert raw == A.deflate_bgzf_host(data)[0] + D.EOF_BLOCK
    (tmp_path / "empty.bin").write_bytes(b"")
    subprocess.run([CLI, "bgzf", "-device", "0", str(tmp_path / "empty.bin"), str(tmp_path / "empty.gz")], check=True, timeout=LIMIT)
    assert (tmp_path / "empty.gz").read_bytes() == D.EOF_BLOCK


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """the reference's regression fixtures (tests/test_gpu_cli_goldens.py): tRex1, 10 k single-end reads and 10 k pairs"""
    wd = tmp_path_factory.mktemp("deflate_chain")
    os.makedirs(wd / "tests")
    os.symlink(os.path.join(ROOT, "tests", "golden", "tRex1.fa"), wd / "tests" / "tRex1.fa")
    subprocess.run([CLI, "idx", "tests/tRex1.fa", "tests/tRex1.idx"], cwd=wd, check=True, timeout=LIMIT)
    common = ["-seed", "1", "-n", "10000", "-m", "0.01", "-b", "0.98", "tests/tRex1.fa"]
    subprocess.run([CLI, "sim", "-single", "-o", "tests/reads"] + common, cwd=wd, check=True, timeout=LIMIT)
    subprocess.run([CLI, "sim", "-o", "tests/reads_pe"] + common, cwd=wd, check=True, timeout=LIMIT)
    return wd


SE = ["-i", "tests/tRex1.idx", "tests/reads_1.fq"]
PE = ["-i", "tests/tRex1.idx", "tests/reads_pe_1.fq", "tests/reads_pe_2.fq"]
TINY = {"ABM_CLI_SLICE_READS": "500"}  # tiny slices: twenty and more device calls a run, blocks far below 0xff00


def run_map(cwd, args, flags=(), **env):
    """`map -B`: (the process, the file(s) written laid end to end, "deflate" of the timing JSON)"""
    r = subprocess.run([CLI, "map", "-B", "-timing", "tests/timing.json", "-o", "tests/out.bam"] + list(flags) + args, cwd=cwd,
                       env=dict(os.environ, **TINY, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LIMIT)
    if r.returncode != 0:
        return r, None, None
    if "-out-parts" in flags:
        raw = b"".join(open(cwd / ("tests/out.bam.part%03d" % k), "rb").read() for k in range(int(flags[flags.index("-out-parts") + 1])))
    else:
        raw = open(cwd / "tests/out.bam", "rb").read()
    return r, raw, json.load(open(cwd / "tests/timing.json"))["deflate"]


def records(raw):
    """the decoded file: (reference names, records) -- what follows the header text, which holds the command line"""
    header, names, recs = B.records_of_stream(B.bgzf_decompress(raw))
    return names, recs


@pytest.mark.parametrize("args", [SE, PE], ids=["single-end", "paired"])
def test_map_deflates_its_records_on_the_device(chain, args):
    r, host, how = run_map(chain, args, ABM_CLI_DEVICE_DEFLATE="0")
    assert r.returncode == 0, r.stdout
    assert how["where"] == "host" and how["device_blocks"] == 0 and how["host_blocks"] > 0 and how["fallback_blocks"] == 0
    r, dev, how = run_map(chain, args, ABM_CLI_DEVICE_DEFLATE="1")
    assert r.returncode == 0, r.stdout
    assert how["where"] == "device" and how["device_blocks"] > 0 and how["host_blocks"] == 0 and how["fallback_blocks"] == 0
    assert dev.endswith(D.EOF_BLOCK)
    assert records(dev) == records(host) and len(records(host)[1]) > 8000


def test_part_files_written_with_the_switch_are_one_bam(chain):
    r, whole, how = run_map(chain, SE, ABM_CLI_DEVICE_DEFLATE="1")
    assert r.returncode == 0, r.stdout
    r, parts, how = run_map(chain, SE, flags=["-out-parts", "2"], ABM_CLI_DEVICE_DEFLATE="1")
    assert r.returncode == 0, r.stdout
    assert how["where"] == "device" and how["device_blocks"] > 0 and how["fallback_blocks"] == 0
    names, recs = records(parts)
    assert names == records(whole)[0] and sorted(recs) == sorted(records(whole)[1])
    assert gzip.decompress(parts) == B.bgzf_decompress(parts)  # one valid gzip file from front to back


def test_other_levels_stay_with_zlib(chain):
    r, six, how = run_map(chain, SE, flags=["-z", "6"], ABM_CLI_DEVICE_DEFLATE="1")
    assert r.returncode == 0, r.stdout
    assert how == {"where": "host", "device_blocks": 0, "host_blocks": how["host_blocks"], "fallback_blocks": 0} and how["host_blocks"] > 0
    members, _ = A.bgzf_scan(six)
    first = six[int(members[1]["at"]):int(members[1]["at"]) + int(members[1]["len"])]
    assert D.walk(first[18:-8])[1]["types"] == {2}  # dynamic codes: zlib's, not the fast encoder's
