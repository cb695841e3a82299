"""BGZF blocks inflated on the GPU (abm_inflate_bgzf, abm_inflate_bgzf_device, `map` with ABM_CLI_DEVICE_INFLATE=1,
`bgzf -d -device`) against Python's zlib, over the fixtures of tests/deflate_tools.py."""
import ctypes as C
import hashlib
import json
import os
import random
import re
import subprocess
import threading

import numpy as np
import pytest

import abismal_amd as A
from tests import deflate_tools as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "abismal_amd", "abismal-amd")
CANARY = 4096


@pytest.fixture(scope="module")
def inflater():
    inf = A.Inflater(0)
    yield inf
    inf.close()


def lay_out(members, gap=0, canary=CANARY):
    """members [(bytes, text_len)] -> (data, descriptors, size of the text buffer): texts end to end from `canary`,
    `gap` bytes apart"""
    blocks = np.zeros(len(members), dtype=A.BGZF_BLOCK_DTYPE)
    at, t = 0, canary
    for k, (m, n) in enumerate(members):
        blocks[k] = (at, t, len(m), n)
        at, t = at + len(m), t + n + gap
    return b"".join(m for m, _ in members), blocks, t - gap + canary if len(members) else 2 * canary


def run_raw(inflater, data, blocks, text_bytes):
    """abm_inflate_bgzf into a buffer prefilled with 0xC5: (return code, text buffer, statuses)"""
    lib = A.load_library()
    buf = np.frombuffer(data, dtype=np.uint8)
    text = np.full(text_bytes, 0xC5, dtype=np.uint8)
    status = np.full(len(blocks), 0xEE, dtype=np.uint8)
    rc = lib.abm_inflate_bgzf(inflater.handle, buf.ctypes.data, len(buf), blocks.ctypes.data, len(blocks), text.ctypes.data, text_bytes, status.ctypes.data)
    return rc, text, status


def untouched(text, blocks):
    """every byte of the text buffer outside the blocks' ranges still holds the canary"""
    mask = np.ones(len(text), dtype=bool)
    for b in blocks:
        mask[int(b["text_at"]):int(b["text_at"]) + int(b["text_len"])] = False
    return bool((text[mask] == 0xC5).all())


def test_every_valid_fixture_alone(inflater):
    for name, member, text in D.valid_fixtures():
        got, status = inflater.inflate(member)
        assert list(status) == [A.INFLATE_OK], (name, status)
        assert got == text, name
        rc, _, _ = run_raw(inflater, *lay_out([(member, len(text))]))
        assert rc == 0, name


@pytest.mark.parametrize("gap", [0, 64])
def test_all_valid_fixtures_in_one_call(inflater, gap):
    valid = list(D.valid_fixtures())
    random.Random(gap).shuffle(valid)
    data, blocks, n = lay_out([(m, len(t)) for _, m, t in valid], gap=gap)
    rc, text, status = run_raw(inflater, data, blocks, n)
    assert rc == 0 and not status.any()
    for (name, _, want), b in zip(valid, blocks):
        assert text[int(b["text_at"]):int(b["text_at"]) + len(want)].tobytes() == want, name
    assert untouched(text, blocks)  # the 4 KB before and after, and the gaps


@pytest.fixture(scope="module")
def many_blocks():
    text = D.fastq_text(1500 * 7919, seed=21)
    members = [(D.bgzf_member(D.deflate(text[at:at + 7919], 1), text[at:at + 7919]), 7919) for at in range(0, len(text), 7919)]
    return text, members


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1500])
def test_block_counts(inflater, many_blocks, n):
    text, members = many_blocks
    data, blocks, size = lay_out(members[:n])
    rc, got, status = run_raw(inflater, data, blocks, size)
    assert rc == 0 and not status.any()
    assert got[CANARY:CANARY + n * 7919].tobytes() == text[:n * 7919]
    assert untouched(got, blocks)


def test_two_inflaters_from_two_threads(many_blocks):
    text, members = many_blocks
    data, blocks, size = lay_out(members)
    out = [None, None]

    def work(k):
        inf = A.Inflater(0)
        try:
            out[k] = run_raw(inf, data, blocks, size)
        finally:
            inf.close()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for rc, got, status in out:
        assert rc == 0 and not status.any()
        assert got[CANARY:CANARY + len(text)].tobytes() == text


def test_device_entry_point_on_a_torch_stream(inflater, many_blocks):
    import torch
    text, members = many_blocks
    data, blocks, size = lay_out(members)
    dev = torch.device("cuda:0")
    d_comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_blocks = torch.frombuffer(bytearray(blocks.tobytes()), dtype=torch.uint8).to(dev)
    d_text = torch.full((size,), 0xC5, dtype=torch.uint8, device=dev)
    d_status = torch.full((len(blocks),), 0xEE, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        inflater.inflate_device(d_comp.data_ptr(), len(data), d_blocks.data_ptr(), len(blocks), d_text.data_ptr(), size, d_status.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert not d_status.cpu().numpy().any()
    got = d_text.cpu().numpy()
    assert got[CANARY:CANARY + len(text)].tobytes() == text
    assert untouched(got, blocks)
    # a descriptor that points outside the buffers named is the kernel's to refuse: HEADER, and nothing written
    bad = blocks[:3].copy()
    bad[1]["at"] = len(data) - 10
    bad[2]["text_at"] = size - 10
    d_bad = torch.frombuffer(bytearray(bad.tobytes()), dtype=torch.uint8).to(dev)
    d_text.fill_(0xC5)
    inflater.inflate_device(d_comp.data_ptr(), len(data), d_bad.data_ptr(), 3, d_text.data_ptr(), size, d_status.data_ptr(), 0)
    torch.cuda.synchronize(dev)
    assert list(d_status.cpu().numpy()[:3]) == [A.INFLATE_OK, A.INFLATE_HEADER, A.INFLATE_HEADER]
    assert untouched(d_text.cpu().numpy(), bad[:1])


def test_host_entry_point_refuses_descriptors_outside_the_buffers(inflater, many_blocks):
    _, members = many_blocks
    data, blocks, size = lay_out(members[:2])
    blocks[1]["text_at"] = size - 100
    rc, text, status = run_raw(inflater, data, blocks, size)
    assert rc not in (0, A.ERR_INFLATE) and "block 1" in A.load_library().abm_last_error().decode()
    assert (text == 0xC5).all() and (status == 0xEE).all()  # nothing was launched


def check_between_neighbours(inflater, member, text_len, expect, original=None):
    (_, left, left_text), (_, right, right_text) = D.valid_fixtures()[0], D.valid_fixtures()[3]
    data, blocks, size = lay_out([(left, len(left_text)), (member, text_len), (right, len(right_text))])
    rc, text, status = run_raw(inflater, data, blocks, size)
    ranges = [text[int(b["text_at"]):int(b["text_at"]) + int(b["text_len"])].tobytes() for b in blocks]
    assert status[0] == status[2] == A.INFLATE_OK and ranges[0] == left_text and ranges[2] == right_text
    assert untouched(text, blocks)
    if expect is None:  # a flipped byte: refused, or harmless
        assert status[1] != 0 or ranges[1] == original
    else:
        assert status[1] == expect
    assert rc == (A.ERR_INFLATE if status[1] else 0)


def test_damaged_fixtures(inflater):
    for name, member, text_len, expect in D.damaged_fixtures():
        try:
            check_between_neighbours(inflater, member, text_len, expect)
        except AssertionError as e:
            raise AssertionError(name) from e
    name, member, text = D.valid_fixtures()[1]
    got, status = inflater.inflate(member)  # the same inflater afterwards
    assert got == text and not status.any()


def test_one_byte_flips(inflater):
    # all 200 in one call, each between two valid members (the call is the unit that costs time, not the block)
    text, flips = D.flip_fixtures()
    (_, left, left_text) = D.valid_fixtures()[2]
    members = [(left, len(left_text))]
    for m in flips:
        members += [(m, len(text)), (left, len(left_text))]
    data, blocks, size = lay_out(members)
    rc, got, status = run_raw(inflater, data, blocks, size)
    refused = 0
    for k, b in enumerate(blocks):
        piece = got[int(b["text_at"]):int(b["text_at"]) + int(b["text_len"])].tobytes()
        if k % 2 == 0:
            assert status[k] == 0 and piece == left_text
        else:
            assert status[k] != 0 or piece == text, k
            refused += status[k] != 0
    assert untouched(got, blocks)
    assert refused > 150 and rc == A.ERR_INFLATE
    rc, _, status = run_raw(inflater, *lay_out([(left, len(left_text))]))
    assert rc == 0 and not status.any()


# ---- through the CLI ---------------------------------------------------------------------------------------------------
def write_bgzf(src, dst, block):
    text = open(src, "rb").read()
    with open(dst, "wb") as o:
        for at in range(0, len(text), block):
            o.write(D.bgzf_member(D.deflate(text[at:at + block], 1), text[at:at + block]))
        o.write(D.EOF_BLOCK)


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """the reference's regression fixtures (tests/test_gpu_cli_goldens.py): tRex1, 10 k single-end reads and 10 k pairs,
    mapped from plain FASTQ; then one directory per BGZF form, the files under the same names (the @PG line has them)"""
    wd = tmp_path_factory.mktemp("bgzf_chain")
    os.makedirs(wd / "plain" / "tests")
    os.symlink(os.path.join(ROOT, "tests", "golden", "tRex1.fa"), wd / "plain" / "tests" / "tRex1.fa")
    subprocess.run([CLI, "idx", "tests/tRex1.fa", "tests/tRex1.idx"], cwd=wd / "plain", check=True)
    common = ["-seed", "1", "-n", "10000", "-m", "0.01", "-b", "0.98", "tests/tRex1.fa"]
    subprocess.run([CLI, "sim", "-single", "-o", "tests/reads"] + common, cwd=wd / "plain", check=True)
    subprocess.run([CLI, "sim", "-o", "tests/reads_pe"] + common, cwd=wd / "plain", check=True)
    for form, block in (("b65280", 0xff00), ("b7919", 7919)):
        os.makedirs(wd / form / "tests")
        os.symlink(wd / "plain" / "tests" / "tRex1.idx", wd / form / "tests" / "tRex1.idx")
        for f in ("reads_1.fq", "reads_pe_1.fq", "reads_pe_2.fq"):
            write_bgzf(wd / "plain" / "tests" / f, wd / form / "tests" / f, block)
    return wd


SE = ["-s", "tests/reads.mstats", "-o", "tests/reads.sam", "-i", "tests/tRex1.idx", "tests/reads_1.fq"]
PE = ["-s", "tests/reads_pe.mstats", "-o", "tests/reads_pe.sam", "-i", "tests/tRex1.idx", "tests/reads_pe_1.fq", "tests/reads_pe_2.fq"]


def run_map(cwd, args, **env):
    r = subprocess.run([CLI, "map", "-timing", "tests/timing.json"] + args, cwd=cwd, env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    outs = [a for a in args if a.endswith(".sam") or a.endswith(".mstats")]
    if r.returncode != 0:
        return r, None, None
    body = [ln for ln in open(cwd / outs[1]) if not ln.startswith("@PG")]
    return r, (body, open(cwd / outs[0]).read()), json.load(open(cwd / "tests/timing.json"))["inflate"]


@pytest.mark.parametrize("form,args,env", [
    ("b65280", SE, {}),
    ("b7919", SE, {"ABM_CLI_CHUNK_BYTES": "30000"}),
    ("b65280", PE, {}),
])
def test_map_inflates_its_input_on_the_device(chain, form, args, env):
    r, plain, how = run_map(chain / "plain", args)
    assert r.returncode == 0, r.stdout
    assert how == {"where": "host", "device_blocks": 0, "host_blocks": 0, "fallback_blocks": 0}
    r, dev, how = run_map(chain / form, args, ABM_CLI_DEVICE_INFLATE="1", **env)
    assert r.returncode == 0, r.stdout
    assert dev == plain and len(plain[0]) > 8000
    assert how["where"] == "device" and how["device_blocks"] > 0 and how["host_blocks"] == 0
    assert how["fallback_blocks"] == 0  # (a decoder that hands valid zlib output back to the host fails here)
    if args is SE:
        # (the reference's own command line, to the letter -- no -timing: the SAM's @PG line carries it)
        subprocess.run([CLI, "map"] + args, cwd=chain / form, env=dict(os.environ, ABM_CLI_DEVICE_INFLATE="1", **env), check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        golden = dict(reversed(line.split()) for line in open(os.path.join(ROOT, "tests", "golden", "md5sum.txt")))
        assert hashlib.md5(open(chain / form / "tests/reads.sam", "rb").read()).hexdigest() == golden["tests/reads.sam"]
    r, host, how = run_map(chain / form, args, ABM_CLI_DEVICE_INFLATE="0", **env)
    assert r.returncode == 0, r.stdout
    assert host == plain
    assert how["where"] == "host" and how["device_blocks"] == 0 and how["host_blocks"] > 0 and how["fallback_blocks"] == 0


def test_map_ends_on_a_damaged_file_with_the_hosts_message(chain, tmp_path):
    src = (chain / "b65280" / "tests" / "reads_1.fq").read_bytes()
    at = len(src) // 2
    (tmp_path / "tests").mkdir()
    os.symlink(chain / "plain" / "tests" / "tRex1.idx", tmp_path / "tests" / "tRex1.idx")
    (tmp_path / "tests" / "reads_1.fq").write_bytes(src[:at] + bytes([src[at] ^ 0x10]) + src[at + 1:])
    said = {}
    for by in ("1", "0"):
        r, _, _ = run_map(tmp_path, SE, ABM_CLI_DEVICE_INFLATE=by)
        assert r.returncode != 0
        said[by] = [ln for ln in r.stdout.splitlines() if "BGZF" in ln]
    assert said["1"] == said["0"] and said["1"]


def test_cli_bgzf_d_on_the_device(tmp_path):
    valid = D.valid_fixtures()
    src = tmp_path / "valid.gz"
    src.write_bytes(b"".join(m for _, m, _ in valid))
    subprocess.run([CLI, "bgzf", "-d", str(src), str(tmp_path / "host.txt")], check=True)
    subprocess.run([CLI, "bgzf", "-d", "-device", "0", str(src), str(tmp_path / "device.txt")], check=True)
    assert (tmp_path / "device.txt").read_bytes() == (tmp_path / "host.txt").read_bytes() == b"".join(t for _, _, t in valid)
    good = valid[0][1]
    n_files = 0
    for name, member, text_len, status in D.damaged_fixtures():
        isize = int.from_bytes(member[-4:], "little")
        if len(member) != int.from_bytes(member[16:18], "little") + 1 or D.zlib_verdict(member, isize) is not None:
            continue  # (as in the host's test: BSIZE has to frame the block, and the damage has to show in a file)
        (tmp_path / "bad.gz").write_bytes(good + member + D.EOF_BLOCK)
        r = subprocess.run([CLI, "bgzf", "-d", "-device", "0", str(tmp_path / "bad.gz"), str(tmp_path / "bad.txt")], stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0, name
        assert re.search(r"at byte %d\b" % len(good), r.stderr), (name, r.stderr)
        n_files += 1
    assert n_files >= 20


def test_the_switch_leaves_plain_input_on_its_parallel_path(chain):
    # plain FASTQ with ABM_CLI_DEVICE_INFLATE set to either value: the same parts as without it (-out-parts needs the
    # mapped, chunk-counted input path), and nothing inflated anywhere
    bodies = {}
    for value in (None, "0", "1"):
        env = {k: v for k, v in os.environ.items() if k != "ABM_CLI_DEVICE_INFLATE"}
        if value is not None:
            env["ABM_CLI_DEVICE_INFLATE"] = value
        r = subprocess.run([CLI, "map", "-out-parts", "2", "-timing", "tests/timing.json", "-o", "tests/parts.sam", "-i", "tests/tRex1.idx", "tests/reads_1.fq"],
                           cwd=chain / "plain", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        bodies[value] = [[ln for ln in open(chain / "plain" / ("tests/parts.sam.part%03d" % k)) if not ln.startswith("@PG")] for k in range(2)]
        t = json.load(open(chain / "plain" / "tests/timing.json"))
        assert t["out_parts"] == 2 and t["inflate"] == {"where": "host", "device_blocks": 0, "host_blocks": 0, "fallback_blocks": 0}
    assert bodies[None] == bodies["0"] == bodies["1"] and sum(len(p) for p in bodies[None]) > 8000
