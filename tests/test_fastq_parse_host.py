"""The FASTQ parser, the parts that need no GPU: the C ABI's surface, abm_fastq_parse_host -- the rules the device kernels
share, run serially -- against an independent restatement of ReadLoader's rules, its errors and capacities, the shared core
on the CPU under sanitizers, and `map` with the switch and no device.

The case table (tests/fastq_cases.py), as test_the_case_table_is_alive counts it: 108 cases, 92 valid and 16 with an error
(the error that wins is an empty name in 4, a read that is too long in 5, a read without a base in 7); in the valid ones
1,068,033 records are cut to empty (1,048,577 of them in the case of seven-byte records), 3 are trimmed at the head only, 2
at the tail only, 11,478 at both ends, and 1,087 lines are longer than a tile.  The test asserts that each of these is
present, not the exact figures."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import abismal_amd as A
from tests import fastq_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "abismal_amd", "abismal-amd")
ENTRY_POINTS = ["abm_fastq_sizes", "abm_fastq_parser_create", "abm_fastq_parser_destroy", "abm_fastq_parse", "abm_fastq_parse_device",
                "abm_fastq_parse_host"]


@pytest.fixture(scope="module")
def lib():
    A.build()
    return A.load_library()


def _last_error(lib):
    return lib.abm_last_error().decode()


# ---- ReadLoader's rules once more (after tests/oracle_binding.read_fastq_like_readloader: bytes, and min_letters) ----------
def restate(text, min_letters):
    """-> dict: names [(at, bytes)], reads [bytes], error (code, line, value) or None -- the first one, where the walk
    stops --, and tallies of what the rules did"""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()  # (the text ends with a newline, or is empty: no line begins there)
    names, reads, error = [], [], None
    tally = dict(empty=0, head=0, tail=0, both=0, long_lines=sum(1 for ln in lines if len(ln) > K.T))
    at = 0
    for k, line in enumerate(lines):
        if k % 4 == 0:
            if not line:
                error = (A.FASTQ_EMPTY_NAME, k, 0)
                break
            cut = min([i for i in (line.find(b" ", 1), line.find(b"\t", 1)) if i >= 0] or [len(line)])
            names.append((at + 1, line[1:cut]))
        elif k % 4 == 1:
            if len(line) >= 32767:
                error = (A.FASTQ_TOO_LONG, k, len(line))
                break
            if len(line) - line.count(b"N") < min_letters:
                read = b""
                tally["empty"] += 1
            else:
                read = line.rstrip(b"N")
                first = min([i for i in (read.find(b) for b in (b"A", b"C", b"G", b"T")) if i >= 0] or [-1])
                if first < 0:
                    error = (A.FASTQ_NO_BASE, k, 0)
                    break
                tail, head = len(read) < len(line), first > 0
                if head or tail:
                    tally["both" if head and tail else "head" if head else "tail"] += 1
                read = read[first:]
            reads.append(read)
        at += len(line) + 1
    n_lines = len(lines)
    return dict(names=names[:len(reads)], reads=reads, error=error, tally=tally, n_records=(n_lines + 2) // 4)


@pytest.fixture(scope="module")
def restated():
    return {name: restate(text, m) for name, text, m in K.cases()}


@pytest.fixture(scope="module")
def parsed(lib):
    return {name: A.fastq_parse_host(text, m) for name, text, m in K.cases()}


# ---- API surface -------------------------------------------------------------------------------------------------------
def test_header_declares_the_fastq_interface():
    h = open(os.path.join(ROOT, "include", "abismal_amd.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, h), name
    assert "typedef struct abm_fastq_parser abm_fastq_parser;" in h
    assert re.search(r"enum\s*{\s*ABM_FASTQ_OK = 0, ABM_FASTQ_EMPTY_NAME, ABM_FASTQ_TOO_LONG, ABM_FASTQ_NO_BASE\s*}", h)
    assert re.search(r"#define\s+ABM_ERR_FASTQ\s+\(-4\)", h)


def test_symbols_are_listed_and_exported(lib):
    for name in ENTRY_POINTS:
        assert name in A.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert (A.FASTQ_OK, A.FASTQ_EMPTY_NAME, A.FASTQ_TOO_LONG, A.FASTQ_NO_BASE, A.ERR_FASTQ) == (0, 1, 2, 3, -4)
    assert A.fastq_sizes() == (K.T, K.S, K.C)
    assert A.FASTQ_INFO_DTYPE.itemsize == 40


def test_null_and_oversized_arguments_are_refused_with_a_text(lib):
    text = (C.c_uint8 * 64)()
    blob = (C.c_uint8 * 64)()
    off = (C.c_uint64 * 8)()
    info = (C.c_uint8 * 40)()
    for call, lead in ((lib.abm_fastq_parse_host, ()), (lib.abm_fastq_parse, (None,))):
        assert call(*lead, None, 64, 44, blob, 64, off, None, None, 4, info) < 0 and "null" in _last_error(lib)
        assert call(*lead, text, 64, 44, None, 64, off, None, None, 4, info) < 0 and "null" in _last_error(lib)
        assert call(*lead, text, 64, 44, blob, 64, None, None, None, 4, info) < 0 and "null" in _last_error(lib)
        assert call(*lead, text, 64, 44, blob, 64, off, None, None, 4, None) < 0 and "null" in _last_error(lib)
        # (refused by its size alone, before the text is looked at)
        assert call(*lead, text, 1 << 32, 44, blob, 64, off, None, None, 4, info) < 0 and "2^32" in _last_error(lib)
    # (the device entry points are refused before anything is launched: no device is needed to see it)
    assert lib.abm_fastq_parse(None, text, 64, 44, blob, 64, off, None, None, 4, info) < 0 and "null" in _last_error(lib)
    assert lib.abm_fastq_parse_device(None, text, 64, 44, blob, 64, off, None, None, 4, info, None) < 0 and "null" in _last_error(lib)
    assert lib.abm_fastq_parser_create(0, None) < 0 and "null" in _last_error(lib)
    lib.abm_fastq_parser_destroy(None)  # (a no-op)


def test_parser_create_fails_loudly_without_a_device(lib):
    h = C.c_void_p()
    if lib.abm_device_count() > 0:  # (on a GPU box the same call succeeds; what it then does is the GPU tests' matter)
        assert lib.abm_fastq_parser_create(0, C.byref(h)) == 0 and h.value
        lib.abm_fastq_parser_destroy(h)
        assert lib.abm_fastq_parser_create(lib.abm_device_count(), C.byref(h)) < 0 and "no such device" in _last_error(lib)
        return
    assert lib.abm_fastq_parser_create(0, C.byref(h)) < 0
    assert "no HIP device" in _last_error(lib) and not h.value
    with pytest.raises(A.AbismalAmdError, match="no HIP device"):
        A.FastqParser(0)


# ---- the case table itself ---------------------------------------------------------------------------------------------
def test_the_case_table_is_alive(restated):
    valid = [r for name, r in restated.items() if not K.is_error(name)]
    errors = {name: r for name, r in restated.items() if K.is_error(name)}
    assert all(r["error"] is None for r in valid) and all(r["error"] is not None for r in errors.values())
    total = {k: sum(r["tally"][k] for r in valid) for k in ("empty", "head", "tail", "both", "long_lines")}
    codes = [r["error"][0] for r in errors.values()]
    print(len(restated), "cases,", len(valid), "valid;", total, "; errors by code:", {c: codes.count(c) for c in (1, 2, 3)})
    assert all(v > 0 for v in total.values()), total
    assert all(codes.count(c) > 0 for c in (A.FASTQ_EMPTY_NAME, A.FASTQ_TOO_LONG, A.FASTQ_NO_BASE))
    # the sizes the kernels can go wrong at
    sizes = {name: len(text) for name, text, m in K.cases()}
    tiles = {-(-n // K.T) for n in sizes.values()}
    assert set(K.TILE_COUNTS) <= tiles and all(s + d in tiles for s in K.SCAN_LEVELS for d in (-1, 0, 1))
    records = {r["n_records"] for r in restated.values()}
    assert set(K.RECORD_COUNTS) <= records and max(records) > K.S * K.C
    assert sizes[K.BIG] > 11 << 20 and restated[K.BIG]["n_records"] > 50000
    assert any(len(r) == K.MAX_READ for v in valid for r in v["reads"])


# ---- the host form against the restatement -------------------------------------------------------------------------------
def test_every_valid_case_gives_the_restated_names_and_reads(restated, parsed):
    checked = 0
    for name, text, m in K.cases():
        if K.is_error(name):
            continue
        want, got = restated[name], parsed[name]
        n = len(want["reads"])
        assert got.info == dict(n_records=n, blob_bytes=sum(map(len, want["reads"])), max_len=max(map(len, want["reads"]), default=0),
                                code=0, line=0, value=0), name
        assert want["n_records"] == n, name
        assert got.blob == b"".join(want["reads"]), name
        lens = np.array([len(r) for r in want["reads"]], dtype=np.uint64)
        assert got.off[0] == 0 and (np.diff(got.off) == lens).all(), name
        assert (got.name_at == np.array([a for a, _ in want["names"]], dtype=np.uint64)).all(), name
        assert (got.name_len == np.array([len(b) for _, b in want["names"]], dtype=np.uint32)).all(), name
        for j in range(0, n, max(1, n // 50)):  # (the positions say which bytes: spelled out for some)
            a, ln = int(got.name_at[j]), int(got.name_len[j])
            assert text[a:a + ln] == want["names"][j][1], (name, j)
        checked += 1
    assert checked > 90


def test_every_error_case_gives_its_code_line_and_value(lib, restated, parsed):
    for name, text, m in K.cases():
        if not K.is_error(name):
            continue
        code, line, value = restated[name]["error"]
        info = parsed[name].info
        assert (info["code"], info["line"], info["value"], info["n_records"]) == (code, line, value, restated[name]["n_records"]), name
    # and the return code, with a message that names the line
    name, text, m = K.by_name("error: 50 x R")
    buf = np.frombuffer(text, dtype=np.uint8)
    blob, off, info = np.zeros(len(text), np.uint8), np.zeros(16, np.uint64), np.zeros(1, A.FASTQ_INFO_DTYPE)
    rc = lib.abm_fastq_parse_host(buf.ctypes.data, len(buf), m, blob.ctypes.data, len(blob), off.ctypes.data, None, None, 15, info.ctypes.data)
    assert rc == A.ERR_FASTQ and "without A/C/G/T at line 5" in _last_error(lib)


def test_a_second_call_returns_the_same(lib, parsed):
    for name in ("4097 records", "a read of 32766 bases, a later tile", "error: too long first, no base later"):
        _, text, m = K.by_name(name)
        again = A.fastq_parse_host(text, m)
        assert again.blob == parsed[name].blob and (again.off == parsed[name].off).all() and again.info == parsed[name].info


# ---- capacity ----------------------------------------------------------------------------------------------------------------
def host_raw(call, text, m, blob_cap, rec_cap, names=True):
    """a parse call into buffers prefilled with 0xC5: (rc, blob, off, name_at, name_len, info as a dict)"""
    buf = np.frombuffer(text, dtype=np.uint8)
    blob = np.full(blob_cap + 64, 0xC5, dtype=np.uint8)
    off = np.full((rec_cap + 1) * 8 + 64, 0xC5, dtype=np.uint8)
    name_at = np.full(rec_cap * 8 + 64, 0xC5, dtype=np.uint8)
    name_len = np.full(rec_cap * 4 + 64, 0xC5, dtype=np.uint8)
    info = np.zeros(1, dtype=A.FASTQ_INFO_DTYPE)
    rc = call(buf.ctypes.data if len(buf) else None, len(buf), m, blob.ctypes.data, blob_cap, off.ctypes.data,
              name_at.ctypes.data if names else None, name_len.ctypes.data if names else None, rec_cap, info.ctypes.data)
    return rc, blob, off, name_at, name_len, {k: int(info[k][0]) for k in A.FASTQ_INFO_DTYPE.names}


def check_capacities(call, who, last_error, text, m, want):
    """exactly enough, one short of either, none at all: what is written and what is not"""
    n, nb = want.info["n_records"], want.info["blob_bytes"]
    rc, blob, off, name_at, name_len, info = host_raw(call, text, m, nb, n)
    assert rc == 0 and info == want.info
    assert blob[:nb].tobytes() == want.blob and (blob[nb:] == 0xC5).all()
    assert off[:(n + 1) * 8].tobytes() == want.off.tobytes() and (off[(n + 1) * 8:] == 0xC5).all()
    assert name_at[:n * 8].tobytes() == want.name_at.tobytes() and (name_at[n * 8:] == 0xC5).all()
    assert name_len[:n * 4].tobytes() == want.name_len.tobytes() and (name_len[n * 4:] == 0xC5).all()
    for blob_cap, rec_cap, word in ((nb - 1, n, "blob_capacity"), (nb, n - 1, "rec_capacity"), (0, n, "blob_capacity"), (nb, 0, "rec_capacity")):
        rc, blob, off, name_at, name_len, info = host_raw(call, text, m, blob_cap, rec_cap)
        assert rc == A.ERR_CAPACITY and word in last_error() and who in last_error()
        assert info == want.info
        assert all((a == 0xC5).all() for a in (blob, off, name_at, name_len))
    rc, blob, off, name_at, name_len, info = host_raw(call, text, m, nb, n, names=False)  # (no names asked for)
    assert rc == 0 and blob[:nb].tobytes() == want.blob and (name_at == 0xC5).all() and (name_len == 0xC5).all()


@pytest.mark.parametrize("name", ["65 records", "4097 records", "a record over three tiles, a later tile"])
def test_a_capacity_too_small_is_reported_and_nothing_is_written(lib, parsed, name):
    _, text, m = K.by_name(name)
    check_capacities(lib.abm_fastq_parse_host, "abm_fastq_parse_host", lambda: _last_error(lib), text, m, parsed[name])


def test_an_empty_text_is_no_record_and_one_offset(lib):
    rc, blob, off, name_at, name_len, info = host_raw(lib.abm_fastq_parse_host, b"", 44, 0, 0)
    assert rc == 0 and info == dict(n_records=0, blob_bytes=0, max_len=0, code=0, line=0, value=0)
    assert off[:8].tobytes() == bytes(8) and (off[8:] == 0xC5).all() and (blob == 0xC5).all()


# ---- the shared core on the CPU, under sanitizers ----------------------------------------------------------------------------
def test_core_parses_every_case_under_sanitizers(restated, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the core's check"
    exe = tmp_path / "fastq_core_check"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "fastq_core_check.cpp")], check=True)
    table = K.cases()
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("<I", len(table)))
        for name, text, m in table:
            r = restated[name]
            f.write(struct.pack("<IQ", m, len(text)) + text)
            if r["error"]:
                code, line, value = r["error"]
                f.write(struct.pack("<QQQQIIB", r["n_records"], 0, line, value, 0, code, 0))
                continue
            reads, n = r["reads"], len(r["reads"])
            f.write(struct.pack("<QQQQIIB", n, sum(map(len, reads)), 0, 0, max(map(len, reads), default=0), 0, 1))
            f.write(b"".join(reads))
            off = np.zeros(n + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(x) for x in reads], dtype=np.uint64)
            f.write(off.tobytes())
            f.write(np.array([a for a, _ in r["names"]], dtype=np.uint64).tobytes())
            f.write(np.array([len(b) for _, b in r["names"]], dtype=np.uint32).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 wrong" % len(table) in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


# ---- through the CLI without a device ----------------------------------------------------------------------------------------
def test_the_switch_is_ignored_on_virtual_gpus(lib, tmp_path):
    fa = os.path.join(ROOT, "tests", "golden", "tRex1.fa")
    subprocess.run([CLI, "idx", fa, str(tmp_path / "t.idx")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.run([CLI, "sim", "-single", "-seed", "3", "-n", "3000", "-o", str(tmp_path / "r"), fa], check=True, stdout=subprocess.DEVNULL)
    files = {}
    for value in (None, "0", "1"):
        env = {k: v for k, v in os.environ.items() if k != "ABM_CLI_DEVICE_PARSE"}
        env.update(ABM_CLI_SLICE_READS="500", ABM_CLI_CHUNK_BYTES="65536")
        if value is not None:
            env["ABM_CLI_DEVICE_PARSE"] = value
        out = tmp_path / "out.sam"  # (one name: the header's command line is then the same too)
        r = subprocess.run([CLI, "map", "-virtual-gpus", "2", "-t", "4", "-batch", "1024", "-timing", str(tmp_path / "t.json"),
                            "-i", str(tmp_path / "t.idx"), "-o", str(out), str(tmp_path / "r_1.fq")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        files[value] = out.read_bytes()
        t = json.load(open(tmp_path / "t.json"))
        assert t["parse"]["where"] == "host" and t["parse"]["device_slices"] == 0 and t["parse"]["fallback_slices"] == 0
        assert t["parse"]["host_slices"] > 0
    assert len(files[None]) > 10000
    assert files[None] == files["0"] == files["1"]
