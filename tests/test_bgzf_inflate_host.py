"""BGZF inflate, the parts that need no GPU: the C ABI's surface, the fixtures' liveness against zlib, abm_bgzf_scan, the
shared decoder core on the CPU under sanitizers, and host inflate through the CLI."""
import ctypes as C
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import abismal_amd as A
from tests import deflate_tools as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "abismal_amd", "abismal-amd")
ENTRY_POINTS = ["abm_bgzf_scan", "abm_inflater_create", "abm_inflater_destroy", "abm_inflate_bgzf", "abm_inflate_bgzf_device"]


@pytest.fixture(scope="module")
def lib():
    A.build()
    return A.load_library()


def _last_error(lib):
    return lib.abm_last_error().decode()


# ---- API surface -------------------------------------------------------------------------------------------------------
def test_header_declares_the_inflate_interface():
    h = open(os.path.join(ROOT, "include", "abismal_amd.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, h), name
    assert "typedef struct abm_inflater abm_inflater;" in h
    assert re.search(r"typedef struct \{ uint64_t at; uint64_t text_at; uint32_t len; uint32_t text_len; \} abm_bgzf_block;", h)
    assert re.search(r"ABM_INFLATE_OK = 0,[^}]*ABM_INFLATE_HEADER,[^}]*ABM_INFLATE_DATA,[^}]*ABM_INFLATE_SIZE,[^}]*ABM_INFLATE_CRC", h, re.S)
    assert re.search(r"#define ABM_ERR_INFLATE \(-3\)", h)


def test_symbols_are_listed_and_exported(lib):
    for name in ENTRY_POINTS:
        assert name in A.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert (A.INFLATE_OK, A.INFLATE_HEADER, A.INFLATE_DATA, A.INFLATE_SIZE, A.INFLATE_CRC, A.ERR_INFLATE) == (0, 1, 2, 3, 4, -3)
    assert A.BGZF_BLOCK_DTYPE.itemsize == 24


def test_null_arguments_are_refused_with_a_text(lib):
    n, t = C.c_uint64(), C.c_uint64()
    buf = (C.c_uint8 * 28).from_buffer_copy(D.EOF_BLOCK)
    assert lib.abm_bgzf_scan(buf, 28, None, 0, None, C.byref(t)) < 0 and "null" in _last_error(lib)
    assert lib.abm_bgzf_scan(None, 28, None, 0, C.byref(n), C.byref(t)) < 0 and "null" in _last_error(lib)
    assert lib.abm_inflater_create(0, None) < 0 and "null" in _last_error(lib)
    st = (C.c_uint8 * 1)()
    blk = np.zeros(1, dtype=A.BGZF_BLOCK_DTYPE)
    assert lib.abm_inflate_bgzf(None, buf, 28, blk.ctypes.data, 1, buf, 0, st) < 0 and "null" in _last_error(lib)
    assert lib.abm_inflate_bgzf_device(None, buf, 28, blk.ctypes.data, 1, buf, 0, st, None) < 0 and "null" in _last_error(lib)
    lib.abm_inflater_destroy(None)  # (a no-op)


def test_inflater_create_fails_loudly_without_a_device(lib):
    h = C.c_void_p()
    if lib.abm_device_count() > 0:  # (on a GPU box the same call succeeds; what it then does is the GPU tests' matter)
        assert lib.abm_inflater_create(0, C.byref(h)) == 0 and h.value
        lib.abm_inflater_destroy(h)
        assert lib.abm_inflater_create(lib.abm_device_count(), C.byref(h)) < 0 and "no such device" in _last_error(lib)
        return
    assert lib.abm_inflater_create(0, C.byref(h)) < 0
    assert "no HIP device" in _last_error(lib) and not h.value
    with pytest.raises(A.AbismalAmdError, match="no HIP device"):
        A.Inflater(0)


# ---- liveness of the fixtures ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walked():
    out = []
    for name, member, text in D.valid_fixtures():
        xlen = int.from_bytes(member[10:12], "little")
        got, tally = D.walk(member[12 + xlen:-8])
        out.append((name, text, got, tally))
    return out


def test_walker_and_zlib_agree_on_every_valid_fixture(walked):
    import zlib
    for (name, member, text), (_, _, got, _) in zip(D.valid_fixtures(), walked):
        xlen = int.from_bytes(member[10:12], "little")
        assert zlib.decompress(member[12 + xlen:-8], -15) == text, name  # (the hand-assembled ones: what the token list says)
        assert got == text, name
        assert D.zlib_verdict(member, len(text)) == text, name


def test_valid_fixtures_cover_what_they_are_meant_to(walked):
    types = set().union(*(t["types"] for _, _, _, t in walked))
    assert types == {0, 1, 2}
    assert any(t["blocks"] >= 3 and t["empty_stored"] for _, _, _, t in walked)
    assert max(t["max_code_len"] for _, _, _, t in walked) == 15
    assert any(t["match_258_at_1"] for _, _, _, t in walked)
    assert max(t["max_dist"] for _, _, _, t in walked) == 32768
    assert max(t["max_match"] for _, _, _, t in walked) == 258
    assert any(t["overlapping"] > 100 for _, _, _, t in walked)
    assert {0, 1, 65280, 65535, 65536} <= {len(text) for _, text, _, _ in walked}
    by_name = {name: t for name, _, _, t in walked}
    assert by_name["fastq Z_FIXED"]["types"] == {1}
    assert by_name["fastq level 0"]["types"] == {0} and by_name["fastq level 0"]["blocks"] == 2
    assert by_name["fastq Z_HUFFMAN_ONLY"]["max_match"] == 0
    assert by_name["fastq flushed twice"]["types"] == {0, 2} and by_name["fastq flushed twice"]["blocks"] == 5
    assert by_name["random bytes"]["types"] == {0}
    assert by_name["fibonacci frequencies"]["max_code_len"] == 15
    assert all(len(member) <= 65536 for _, member, _ in D.valid_fixtures())


def test_zlib_refuses_every_damaged_fixture():
    causes = {D.HEADER: 0, D.DATA: 0, D.SIZE: 0, D.CRC: 0}
    for name, member, text_len, status in D.damaged_fixtures():
        assert D.zlib_verdict(member, text_len) is None, name
        causes[status] += 1
    assert causes[D.HEADER] >= 5 and causes[D.DATA] >= 11 and causes[D.SIZE] >= 2 and causes[D.CRC] >= 1
    text, flips = D.flip_fixtures()
    assert len(flips) == 200
    refused = 0
    for m in flips:
        v = D.zlib_verdict(m, len(text))
        assert v is None or v == text
        refused += v is None
    assert refused > 150


# ---- abm_bgzf_scan -------------------------------------------------------------------------------------------------------
def _bgzf_file(text, block):
    out = b""
    for at in range(0, len(text), block):
        out += D.bgzf_member(D.deflate(text[at:at + block], 1), text[at:at + block])
    return out


@pytest.mark.parametrize("block", [0xff00, 7919])
def test_scan_lists_every_block(lib, block):
    text = D.fastq_text(200000)
    data = _bgzf_file(text[:100000], block) + D.EOF_BLOCK + D.EOF_BLOCK + _bgzf_file(text[100000:], block) + D.EOF_BLOCK
    blocks, n_text = A.bgzf_scan(data)
    assert n_text == len(text)
    assert len(blocks) == 2 * -(-100000 // block) + 3
    assert int((blocks["text_len"] == 0).sum()) == 3
    at = t = 0
    for b in blocks:
        assert (int(b["at"]), int(b["text_at"])) == (at, t)
        assert D.zlib_verdict(data[at:at + int(b["len"])], int(b["text_len"])) == text[t:t + int(b["text_len"])]
        at, t = at + int(b["len"]), t + int(b["text_len"])
    assert at == len(data)
    assert A.bgzf_scan(b"")[1] == 0 and len(A.bgzf_scan(b"")[0]) == 0


def test_scan_refuses_a_file_cut_inside_a_header_or_a_block(lib):
    data = _bgzf_file(D.fastq_text(20000), 7919)
    blocks, _ = A.bgzf_scan(data)
    second = int(blocks[1]["at"])
    for cut in (second + 7, second + 17, second + 100, len(data) - 1):
        # (the cut data in a buffer of exactly its size)
        with pytest.raises(A.AbismalAmdError, match="at byte %d" % (second if cut < int(blocks[2]["at"]) else int(blocks[-1]["at"]))):
            A.bgzf_scan(bytes(data[:cut]))
    with pytest.raises(A.AbismalAmdError, match="at byte 0"):
        A.bgzf_scan(b"@read\nACGT\n+\nFFFF\n" * 4)


def test_out_of_range_descriptors_are_refused_before_any_launch(lib):
    # (descriptors are checked on the host before the inflater is touched: no device is needed to see it)
    member = D.valid_fixtures()[0][1]
    buf = (C.c_uint8 * len(member)).from_buffer_copy(member)
    text = (C.c_uint8 * 65280)()
    st = (C.c_uint8 * 2)()
    blk = np.zeros(2, dtype=A.BGZF_BLOCK_DTYPE)
    for bad, what in [((1, 0, len(member), 65280), "block 1 lies outside the compressed bytes"),
                      ((2 ** 63, 0, len(member), 65280), "block 1 lies outside the compressed bytes"),
                      ((0, 1, len(member), 65280), "the text of block 1 lies outside the text buffer"),
                      ((0, 2 ** 64 - 1, len(member), 2), "the text of block 1 lies outside the text buffer")]:
        blk[0] = (0, 0, len(member), 65280)
        blk[1] = bad
        assert lib.abm_inflate_bgzf(None, buf, len(member), blk.ctypes.data, 2, text, 65280, st) < 0
        assert what in _last_error(lib), _last_error(lib)


# ---- the shared core on the CPU, under sanitizers -----------------------------------------------------------------------
def test_core_inflates_every_fixture_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the core's check"
    exe = tmp_path / "inflate_core_check"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "inflate_core_check.cpp")], check=True)
    n = D.write_core_fixtures(tmp_path / "fixtures.bin")
    r = subprocess.run([str(exe), str(tmp_path / "fixtures.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d members, 0 wrong" % n in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


# ---- host inflate through the CLI ------------------------------------------------------------------------------------------
def test_cli_bgzf_d_on_the_host(lib, tmp_path):
    valid = D.valid_fixtures()
    src = tmp_path / "valid.gz"
    src.write_bytes(b"".join(m for _, m, _ in valid))
    subprocess.run([CLI, "bgzf", "-d", str(src), str(tmp_path / "valid.txt")], check=True)
    assert (tmp_path / "valid.txt").read_bytes() == gzip.open(src).read() == b"".join(t for _, _, t in valid)
    # round trip of the CLI's own blocks
    subprocess.run([CLI, "bgzf", str(tmp_path / "valid.txt"), str(tmp_path / "again.gz")], check=True)
    subprocess.run([CLI, "bgzf", "-d", str(tmp_path / "again.gz"), str(tmp_path / "again.txt")], check=True)
    assert (tmp_path / "again.txt").read_bytes() == (tmp_path / "valid.txt").read_bytes()
    good = valid[0][1]
    for name, member, text_len, status in D.damaged_fixtures():
        isize = int.from_bytes(member[-4:], "little")
        if len(member) != int.from_bytes(member[16:18], "little") + 1 or D.zlib_verdict(member, isize) is not None:
            continue  # (a file is walked by its headers: BSIZE has to frame the block; and a member that is damaged only against its descriptor is none in a file)
        bad = tmp_path / "bad.gz"
        bad.write_bytes(good + member + D.EOF_BLOCK)
        r = subprocess.run([CLI, "bgzf", "-d", str(bad), str(tmp_path / "bad.txt")], stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0, name
        assert re.search(r"at byte %d\b" % len(good), r.stderr), (name, r.stderr)


def test_the_switch_leaves_plain_input_on_its_parallel_path(lib, tmp_path):
    # ABM_CLI_DEVICE_INFLATE concerns BGZF input alone: plain FASTQ stays on the mapped, chunk-counted path with either
    # value -- -out-parts, which only that path serves, still works and writes the same parts
    fa = os.path.join(ROOT, "tests", "golden", "tRex1.fa")
    subprocess.run([CLI, "idx", fa, str(tmp_path / "t.idx")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.run([CLI, "sim", "-single", "-seed", "3", "-n", "3000", "-o", str(tmp_path / "r"), fa], check=True, stdout=subprocess.DEVNULL)
    bodies = {}
    for value in (None, "0", "1"):
        env = {k: v for k, v in os.environ.items() if k != "ABM_CLI_DEVICE_INFLATE"}
        env.update(ABM_CLI_SLICE_READS="500", ABM_CLI_CHUNK_BYTES="65536")
        if value is not None:
            env["ABM_CLI_DEVICE_INFLATE"] = value
        out = tmp_path / ("out_%s.sam" % value)
        r = subprocess.run([CLI, "map", "-virtual-gpus", "2", "-t", "4", "-batch", "1024", "-out-parts", "2", "-timing", str(tmp_path / "t.json"),
                            "-i", str(tmp_path / "t.idx"), "-o", str(out), str(tmp_path / "r_1.fq")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        parts = [open("%s.part%03d" % (out, k)).read() for k in range(2)]
        assert all(len(p) > 10000 for p in parts)
        bodies[value] = [[ln for ln in p.split("\n") if not ln.startswith("@PG")] for p in parts]
        import json
        t = json.load(open(tmp_path / "t.json"))
        assert t["out_parts"] == 2 and t["inflate"] == {"where": "host", "device_blocks": 0, "host_blocks": 0, "fallback_blocks": 0}
    assert bodies[None] == bodies["0"] == bodies["1"]
