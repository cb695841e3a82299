"""FASTQ text parsed on the GPU (abm_fastq_parse, abm_fastq_parse_device, `map` with ABM_CLI_DEVICE_PARSE=1) against
abm_fastq_parse_host -- which tests/test_fastq_parse_host.py holds against a restatement of ReadLoader's rules -- over the
cases of tests/fastq_cases.py; and inflate -> parse -> map on one stream against the oracle."""
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import abismal_amd as A
from tests import deflate_tools as D
from tests import fastq_cases as K
from tests import oracle_binding as ob

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "abismal_amd", "abismal-amd")
GOLD = os.path.join(ROOT, "tests", "golden")
CANARY = 4096
INFO_BYTES = A.FASTQ_INFO_DTYPE.itemsize


@pytest.fixture(scope="module")
def parser():
    p = A.FastqParser(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def want():
    """{case: FastqReads of abm_fastq_parse_host}"""
    return {name: A.fastq_parse_host(text, m) for name, text, m in K.cases()}


class Framed:
    """the four output arrays, each inside a larger buffer of 0xC5 with CANARY bytes on either side"""

    def __init__(self, blob_cap, rec_cap):
        self.sizes = dict(blob=blob_cap, off=(rec_cap + 1) * 8, name_at=rec_cap * 8, name_len=rec_cap * 4)
        self.buf = {k: np.full(n + 2 * CANARY, 0xC5, dtype=np.uint8) for k, n in self.sizes.items()}

    def ptr(self, k):
        return self.buf[k].ctypes.data + CANARY

    def inner(self, k, n=None):
        return self.buf[k][CANARY:CANARY + (self.sizes[k] if n is None else n)]

    def untouched_from(self, k, n):
        """everything but the array's first n bytes still holds the canary"""
        b = self.buf[k]
        return bool((b[:CANARY] == 0xC5).all() and (b[CANARY + n:] == 0xC5).all())


def run_raw(parser, text, m, blob_cap, rec_cap, names=True):
    """abm_fastq_parse into framed buffers: (rc, Framed, info as a dict)"""
    lib = A.load_library()
    buf = np.frombuffer(text, dtype=np.uint8)
    f = Framed(blob_cap, rec_cap)
    info = np.zeros(1, dtype=A.FASTQ_INFO_DTYPE)
    rc = lib.abm_fastq_parse(parser.handle, buf.ctypes.data if len(buf) else None, len(buf), m, f.ptr("blob"), blob_cap, f.ptr("off"),
                             f.ptr("name_at") if names else None, f.ptr("name_len") if names else None, rec_cap, info.ctypes.data)
    return rc, f, {k: int(info[k][0]) for k in A.FASTQ_INFO_DTYPE.names}


def same_outputs(f, w):
    """the framed arrays hold exactly FastqReads w and nothing else was written"""
    n, nb = w.info["n_records"], w.info["blob_bytes"]
    return (f.inner("blob", nb).tobytes() == w.blob and f.untouched_from("blob", nb)
            and f.inner("off", (n + 1) * 8).tobytes() == w.off.tobytes() and f.untouched_from("off", (n + 1) * 8)
            and f.inner("name_at", n * 8).tobytes() == w.name_at.tobytes() and f.untouched_from("name_at", n * 8)
            and f.inner("name_len", n * 4).tobytes() == w.name_len.tobytes() and f.untouched_from("name_len", n * 4))


# ---- every case alone ------------------------------------------------------------------------------------------------------
def test_every_valid_case_equals_the_host_form(parser, want):
    bad, n_cases = [], 0
    for name, text, m in K.cases():
        if K.is_error(name):
            continue
        w = want[name]
        rc, f, info = run_raw(parser, text, m, w.info["blob_bytes"], w.info["n_records"])
        if rc != 0 or info != w.info or not same_outputs(f, w):
            bad.append((name, rc, info, w.info))
        n_cases += 1
    assert not bad, "%d of %d cases differ; first: %s" % (len(bad), n_cases, bad[:3])
    assert n_cases > 90


def test_every_error_case_gives_the_hosts_code_line_and_value(parser, want):
    bad = []
    for name, text, m in K.cases():
        if not K.is_error(name):
            continue
        w = want[name]
        assert w.info["code"] != 0
        # room for everything the text could give: the outputs hold unspecified bytes INSIDE their ranges
        n, nb = w.info["n_records"], len(text)
        rc, f, info = run_raw(parser, text, m, nb, n)
        ok = rc == A.ERR_FASTQ and info == w.info
        ok = ok and f.untouched_from("blob", nb) and f.untouched_from("off", (n + 1) * 8) and f.untouched_from("name_at", n * 8) and f.untouched_from("name_len", n * 4)
        if not ok:
            bad.append((name, rc, info, w.info))
    assert not bad, bad[:3]


@pytest.mark.parametrize("name", ["65 records", "4097 records", "a record over three tiles, a later tile", "a read of 32766 bases, record 0"])
def test_capacities_exact_one_short_and_zero(parser, want, name):
    _, text, m = K.by_name(name)
    w = want[name]
    n, nb = w.info["n_records"], w.info["blob_bytes"]
    rc, f, info = run_raw(parser, text, m, nb, n)
    assert rc == 0 and info == w.info and same_outputs(f, w)
    for blob_cap, rec_cap, word in ((nb - 1, n, "blob_capacity"), (nb, n - 1, "rec_capacity"), (0, n, "blob_capacity"), (nb, 0, "rec_capacity")):
        rc, f, info = run_raw(parser, text, m, blob_cap, rec_cap)
        assert rc == A.ERR_CAPACITY and word in A.load_library().abm_last_error().decode()
        assert info == w.info  # (what is needed)
        assert all((b == 0xC5).all() for b in f.buf.values())
    rc, f, info = run_raw(parser, text, m, nb, n, names=False)
    assert rc == 0 and f.inner("blob", nb).tobytes() == w.blob and all((f.buf[k] == 0xC5).all() for k in ("name_at", "name_len"))


def test_an_empty_text_is_no_record_and_one_offset(parser):
    rc, f, info = run_raw(parser, b"", 44, 0, 0)
    assert rc == 0 and info == dict(n_records=0, blob_bytes=0, max_len=0, code=0, line=0, value=0)
    assert f.inner("off", 8).tobytes() == bytes(8) and f.untouched_from("off", 8) and (f.buf["blob"] == 0xC5).all()


# ---- the device entry point: any alignment of the text, capacities enforced by the kernels ----------------------------------
def device_parse(parser, text, m, shift, blob_cap, rec_cap, stream=None):
    """abm_fastq_parse_device with the text `shift` bytes into its buffer and every output framed in 0xC5 on the device:
    ({name: whole buffer as numpy}, info as a dict)"""
    import torch
    dev = torch.device("cuda:0")
    d_text = torch.full((len(text) + shift + 16,), 0x0a, dtype=torch.uint8, device=dev)  # (newlines around it: reading outside shows)
    if len(text):
        d_text[shift:shift + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    sizes = dict(blob=blob_cap, off=(rec_cap + 1) * 8, name_at=rec_cap * 8, name_len=rec_cap * 4, info=INFO_BYTES)
    d = {k: torch.full((n + 2 * CANARY,), 0xC5, dtype=torch.uint8, device=dev) for k, n in sizes.items()}
    stream = stream or torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        parser.parse_device(d_text.data_ptr() + shift, len(text), m, d["blob"].data_ptr() + CANARY, blob_cap, d["off"].data_ptr() + CANARY,
                            d["name_at"].data_ptr() + CANARY, d["name_len"].data_ptr() + CANARY, rec_cap, d["info"].data_ptr() + CANARY, stream.cuda_stream)
    stream.synchronize()
    out = {k: v.cpu().numpy() for k, v in d.items()}
    info = out["info"][CANARY:CANARY + INFO_BYTES].view(A.FASTQ_INFO_DTYPE)
    return out, {k: int(info[k][0]) for k in A.FASTQ_INFO_DTYPE.names}


def framed_equal(buf, payload):
    return buf[CANARY:CANARY + len(payload)].tobytes() == payload and bool((buf[:CANARY] == 0xC5).all() and (buf[CANARY + len(payload):] == 0xC5).all())


ALIGNMENT_CASES = ["4097 records", "a name line of 9000 bytes, a later tile", "a name line of 20000 bytes without a blank, record 0",
                   "a read of 32766 bases, a later tile", "a read of 32766 bases, Ns at both ends, record 0"]


@pytest.mark.parametrize("shift", [0, 1, 3, 7, 15])
def test_device_entry_point_on_a_torch_stream_at_any_alignment(parser, want, shift):
    for name in ALIGNMENT_CASES:
        _, text, m = K.by_name(name)
        w = want[name]
        n, nb = w.info["n_records"], w.info["blob_bytes"]
        out, info = device_parse(parser, text, m, shift, nb, n)
        assert info == w.info, name
        assert framed_equal(out["blob"], w.blob) and framed_equal(out["off"], w.off.tobytes()), name
        assert framed_equal(out["name_at"], w.name_at.tobytes()) and framed_equal(out["name_len"], w.name_len.tobytes()), name
        assert framed_equal(out["info"], out["info"][CANARY:CANARY + INFO_BYTES].tobytes()), name


def test_device_entry_point_writes_nothing_beyond_its_capacities(parser, want):
    name = "4097 records"
    _, text, m = K.by_name(name)
    w = want[name]
    n, nb = w.info["n_records"], w.info["blob_bytes"]
    # a blob one byte short: everything else whole, the last byte left out, *d_info says what there was
    out, info = device_parse(parser, text, m, 5, nb - 1, n)
    assert info == w.info
    assert framed_equal(out["blob"], w.blob[:-1]) and framed_equal(out["off"], w.off.tobytes()) and framed_equal(out["name_at"], w.name_at.tobytes())
    # no blob at all
    out, info = device_parse(parser, text, m, 5, 0, n)
    assert info == w.info and (out["blob"] == 0xC5).all() and framed_equal(out["off"], w.off.tobytes())
    # records one short, and none: only the count comes back
    for rec_cap in (n - 1, 0):
        out, info = device_parse(parser, text, m, 5, nb, rec_cap)
        assert info == dict(n_records=n, blob_bytes=0, max_len=0, code=0, line=0, value=0)
        assert all((out[k] == 0xC5).all() for k in ("blob", "off", "name_at", "name_len"))
    # an error case through the device form: the same outcome, nothing outside the ranges
    name = "error: too long first, no base later"
    _, text, m = K.by_name(name)
    w = want[name]
    out, info = device_parse(parser, text, m, 3, len(text), w.info["n_records"])
    assert info == w.info
    assert all((out[k][:CANARY] == 0xC5).all() and (out[k][-CANARY:] == 0xC5).all() for k in out)


# ---- parsers side by side, and one parser over a large text and then a small one ------------------------------------------
def test_two_parsers_from_two_threads(want):
    _, text, m = K.by_name(K.BIG)
    w = want[K.BIG]
    out = [None, None]

    def work(k):
        p = A.FastqParser(0)
        try:
            out[k] = run_raw(p, text, m, w.info["blob_bytes"], w.info["n_records"])
        finally:
            p.close()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for rc, f, info in out:
        assert rc == 0 and info == w.info and same_outputs(f, w)


def test_a_grown_workspace_leaves_nothing_stale_behind(want):
    p = A.FastqParser(0)
    try:
        for name in (K.BIG, "2 records", "a name line alone", "63 records", K.BIG, "error: 50 x R", "65 records"):
            _, text, m = K.by_name(name)
            w = want[name]
            got = p.parse(text, m)
            assert got.info == w.info, name
            if not K.is_error(name):
                assert got.blob == w.blob and (got.off == w.off).all() and (got.name_at == w.name_at).all() and (got.name_len == w.name_len).all(), name
    finally:
        p.close()


# ---- inflate -> parse -> map on one stream, nothing copied to the host in between ------------------------------------------
def as_bgzf(text, block=0xff00):
    return b"".join(D.bgzf_member(D.deflate(text[at:at + block], 1), text[at:at + block]) for at in range(0, len(text), block))


class Resident:
    """one FASTQ file as BGZF in HBM, with the buffers its text, reads and offsets go to"""

    def __init__(self, path, dev):
        import torch
        self.text = open(path, "rb").read()
        self.host = A.fastq_parse_host(self.text)  # (the test knows n, max_len and the sizes from the host form)
        data = as_bgzf(self.text)
        blocks, text_bytes = A.bgzf_scan(data)
        assert text_bytes == len(self.text)
        self.n_blocks, self.comp_bytes = len(blocks), len(data)
        self.d_comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        self.d_blocks = torch.frombuffer(bytearray(blocks.tobytes()), dtype=torch.uint8).to(dev)
        self.d_text = torch.zeros(text_bytes, dtype=torch.uint8, device=dev)
        self.d_status = torch.full((len(blocks),), 0xEE, dtype=torch.uint8, device=dev)
        n = self.host.info["n_records"]
        self.d_blob = torch.zeros(max(1, self.host.info["blob_bytes"]), dtype=torch.uint8, device=dev)
        self.d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self.d_info = torch.zeros(INFO_BYTES, dtype=torch.uint8, device=dev)

    def enqueue(self, inflater, parser, stream):
        inflater.inflate_device(self.d_comp.data_ptr(), self.comp_bytes, self.d_blocks.data_ptr(), self.n_blocks, self.d_text.data_ptr(), len(self.text),
                                self.d_status.data_ptr(), stream.cuda_stream)
        parser.parse_device(self.d_text.data_ptr(), len(self.text), 44, self.d_blob.data_ptr(), self.host.info["blob_bytes"], self.d_off.data_ptr(), None, None,
                            self.host.info["n_records"], self.d_info.data_ptr(), stream.cuda_stream)

    def check(self):
        assert not self.d_status.cpu().numpy().any()
        info = self.d_info.cpu().numpy().view(A.FASTQ_INFO_DTYPE)
        assert {k: int(info[k][0]) for k in A.FASTQ_INFO_DTYPE.names} == self.host.info
        assert self.d_blob.cpu().numpy()[:self.host.info["blob_bytes"]].tobytes() == self.host.blob


def slots_as_blob(d_cig, d_n):
    """fixed CIGAR slots -> (ops end to end, n + 1 offsets), as the batch entry points return them"""
    cn = d_n.cpu().numpy().astype(np.int64)
    dc = d_cig.cpu().numpy().view(np.uint32)
    off = np.zeros(len(cn) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(cn)
    blob = np.concatenate([dc[i, :cn[i]] for i in range(len(cn))]) if len(cn) else np.zeros(0, np.uint32)
    return blob, off


def test_chain_inflate_parse_map_single_end(oracle, trex_index, workdir, parser):
    import torch
    from tests.test_gpu_se_parity import compare_se
    prefix = os.path.join(workdir, "fastq_chain_se")
    oracle.simulate(os.path.join(GOLD, "tRex1.fa"), prefix, 10000, single_end=True)
    _, reads = ob.read_fastq_like_readloader(prefix + "_1.fq")
    dev = torch.device("cuda:0")
    r = Resident(prefix + "_1.fq", dev)
    n, L = r.host.info["n_records"], r.host.info["max_len"]
    assert n == len(reads) == 10000
    stride = L + 2
    d_res = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    d_cig = torch.zeros((n, stride), dtype=torch.int32, device=dev)
    d_n = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    ix = A.Index(trex_index)
    ctx = A.Context(ix, 0)
    inflater = A.Inflater(0)
    try:
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            r.enqueue(inflater, parser, stream)
            ctx.map_se_device(A.SE_T_RICH, A.Params(), n, r.d_blob.data_ptr(), r.d_off.data_ptr(), L, d_res.data_ptr(), d_cig.data_ptr(), stride,
                              d_n.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        r.check()
        assert int(d_st.item()) == 0
        res = d_res.cpu().numpy().view(A.HIT_DTYPE).reshape(-1)
        cig, cig_off = slots_as_blob(d_cig, d_n)
    finally:
        inflater.close()
        ctx.close()
        ix.close()
    oix = oracle.index_load(trex_index)
    try:
        o_res, o_cig, o_cig_n, _ = oracle.map_se(oix, reads, mode=0, threads=8)
    finally:
        oracle.index_free(oix)
    compare_se(res, cig, cig_off, o_res, o_cig, o_cig_n, reads, "inflate -> parse -> map, single end")
    assert int((res["pos"] != 0).sum()) > 0.85 * sum(1 for x in reads if x)


def test_chain_inflate_parse_map_pairs(oracle, trex_index, workdir, parser):
    import torch
    from tests.test_gpu_pe_parity import compare_pe
    prefix = os.path.join(workdir, "fastq_chain_pe")
    oracle.simulate(os.path.join(GOLD, "tRex1.fa"), prefix, 10000)
    _, r1 = ob.read_fastq_like_readloader(prefix + "_1.fq")
    _, r2 = ob.read_fastq_like_readloader(prefix + "_2.fq")
    dev = torch.device("cuda:0")
    ends = [Resident(prefix + "_1.fq", dev), Resident(prefix + "_2.fq", dev)]
    n = ends[0].host.info["n_records"]
    assert n == ends[1].host.info["n_records"] == len(r1) == 10000
    L = max(e.host.info["max_len"] for e in ends)
    stride = L + 2
    pair_bytes = A.PAIR_DTYPE.itemsize
    d_pair = torch.zeros(n * pair_bytes, dtype=torch.uint8, device=dev)
    d_se = [torch.zeros((n, 2), dtype=torch.int32, device=dev) for _ in range(2)]
    d_cig = [torch.zeros((n, stride), dtype=torch.int32, device=dev) for _ in range(2)]
    d_n = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)]
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = A.load_library()
    ix = A.Index(trex_index)
    ctx = A.Context(ix, 0)
    inflater = A.Inflater(0)
    params = A.Params()
    try:
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            for e in ends:  # (both ends by one parser: its scratch is reused in stream order)
                e.enqueue(inflater, parser, stream)
            rc = lib.abm_map_pe_device(ctx.handle, A.PE_NORMAL, C.byref(params), n, ends[0].d_blob.data_ptr(), ends[0].d_off.data_ptr(),
                                       ends[1].d_blob.data_ptr(), ends[1].d_off.data_ptr(), L, d_pair.data_ptr(), d_se[0].data_ptr(), d_se[1].data_ptr(),
                                       d_cig[0].data_ptr(), d_cig[1].data_ptr(), stride, d_n[0].data_ptr(), d_n[1].data_ptr(), d_st.data_ptr(),
                                       stream.cuda_stream)
            assert rc == 0, lib.abm_last_error().decode()
        stream.synchronize()
        for e in ends:
            e.check()
        assert int(d_st.item()) == 0
        pairs = d_pair.cpu().numpy().view(A.PAIR_DTYPE)
        se = [d.cpu().numpy().view(A.HIT_DTYPE).reshape(-1) for d in d_se]
        gpu = (pairs, se[0], se[1], slots_as_blob(d_cig[0], d_n[0]), slots_as_blob(d_cig[1], d_n[1]))
    finally:
        inflater.close()
        ctx.close()
        ix.close()
    oix = oracle.index_load(trex_index)
    try:
        orc = oracle.map_pe(oix, r1, r2, mode=0, threads=8)
    finally:
        oracle.index_free(oix)
    compare_pe(gpu, orc, "inflate -> parse -> map, pairs")
    assert int((pairs["r1"]["pos"] != 0).sum()) > 0.3 * n


# ---- through the CLI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_dir(tmp_path_factory):
    """the reference's regression fixtures (tests/test_gpu_cli_goldens.py): tRex1, 10 k single-end reads and 10 k pairs"""
    wd = tmp_path_factory.mktemp("fastq_cli")
    os.makedirs(wd / "tests")
    os.symlink(os.path.join(GOLD, "tRex1.fa"), wd / "tests" / "tRex1.fa")
    subprocess.run([CLI, "idx", "tests/tRex1.fa", "tests/tRex1.idx"], cwd=wd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    common = ["-seed", "1", "-n", "10000", "-m", "0.01", "-b", "0.98", "tests/tRex1.fa"]
    subprocess.run([CLI, "sim", "-single", "-o", "tests/reads"] + common, cwd=wd, check=True, stdout=subprocess.DEVNULL)
    subprocess.run([CLI, "sim", "-o", "tests/reads_pe"] + common, cwd=wd, check=True, stdout=subprocess.DEVNULL)
    return wd


SE = ["-s", "tests/out.mstats", "-o", "tests/out.sam", "-i", "tests/tRex1.idx"]


def run_map(cwd, args, **env):
    """`map` -> (process, (SAM lines without @PG, statistics) or None, the timing file's "parse" entry or None)"""
    timing = cwd / "tests" / "timing.json"
    if timing.exists():
        timing.unlink()
    r = subprocess.run([CLI, "map", "-timing", "tests/timing.json"] + SE + args, cwd=cwd, env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    how = json.load(open(timing))["parse"] if timing.exists() else None
    if r.returncode != 0:
        return r, None, how
    body = [ln for ln in open(cwd / "tests/out.sam") if not ln.startswith("@PG")]
    return r, (body, open(cwd / "tests/out.mstats").read()), how


def both_ways(cwd, args, **env):
    r, host, how = run_map(cwd, args, ABM_CLI_DEVICE_PARSE="0", **env)
    assert r.returncode == 0, r.stdout
    assert how["where"] == "host" and how["device_slices"] == 0 and how["fallback_slices"] == 0 and how["host_slices"] > 0
    r, dev, how = run_map(cwd, args, ABM_CLI_DEVICE_PARSE="1", **env)
    assert r.returncode == 0, r.stdout
    assert dev == host
    assert how["where"] == "device" and how["device_slices"] > 0 and how["host_slices"] == 0 and how["fallback_slices"] == 0  # every slice on the device
    return host


@pytest.mark.parametrize("reads,env", [
    (["tests/reads_1.fq"], {}),
    (["tests/reads_pe_1.fq", "tests/reads_pe_2.fq"], {}),
    (["tests/reads_1.fq"], {"ABM_CLI_SLICE_READS": "500", "ABM_CLI_CHUNK_BYTES": "65536"}),
    (["tests/reads_pe_1.fq", "tests/reads_pe_2.fq"], {"ABM_CLI_SLICE_READS": "500", "ABM_CLI_CHUNK_BYTES": "65536"}),
])
def test_map_parses_its_input_on_the_device(cli_dir, reads, env):
    host = both_ways(cli_dir, reads, **env)
    assert len(host[0]) > 8000


def test_map_inflates_and_parses_on_the_device(cli_dir):
    text = open(cli_dir / "tests" / "reads_1.fq", "rb").read()
    (cli_dir / "tests" / "reads_bgzf.fq").write_bytes(as_bgzf(text) + D.EOF_BLOCK)
    r, plain, _ = run_map(cli_dir, ["tests/reads_1.fq"])
    assert r.returncode == 0, r.stdout
    # (the @PG line aside, which names the input, BGZF input gives what plain input gives)
    host = both_ways(cli_dir, ["tests/reads_bgzf.fq"], ABM_CLI_DEVICE_INFLATE="1")
    assert host == plain and len(host[0]) > 8000


def test_map_device_parse_on_ghost_lengths_and_a_longest_read(cli_dir):
    # reads of 44-46 bases (what a read finds past its end comes from the reads before it: the slices' tails must be the
    # host's), and one of 32766
    rng = np.random.default_rng(5)
    genome = "".join(ln.strip() for ln in open(cli_dir / "tests" / "tRex1.fa") if not ln.startswith(">")).upper()
    recs = []
    for i in range(4000):
        L = int(rng.integers(44, 47)) if i % 3 else int(rng.integers(60, 140))
        at = int(rng.integers(0, len(genome) - 200))
        recs.append(K.rec(b"g%d" % i, genome[at:at + L].replace("C", "T").encode()))
    (cli_dir / "tests" / "ghost.fq").write_bytes(b"".join(recs))
    both_ways(cli_dir, ["tests/ghost.fq"], ABM_CLI_SLICE_READS="500", ABM_CLI_CHUNK_BYTES="65536")
    at = 1000
    recs[100] = K.rec(b"longest", genome[at:at + K.MAX_READ].replace("C", "T").encode())
    (cli_dir / "tests" / "longest.fq").write_bytes(b"".join(recs[:300]))
    both_ways(cli_dir, ["tests/longest.fq"])


def test_map_ends_on_a_bad_input_with_the_hosts_message(cli_dir):
    good = open(cli_dir / "tests" / "reads_1.fq", "rb").read()
    cut = good.index(b"\n@", len(good) // 2) + 1  # a record's first byte
    bad = {
        "empty_name.fq": good[:cut] + b"\n" + good[cut:],
        "too_long.fq": good[:cut] + K.rec(b"big", (b"ACGT" * 8192)[:K.MAX_READ + 1]) + good[cut:],  # 32767 bytes
    }
    for name, text in bad.items():
        (cli_dir / "tests" / name).write_bytes(text)
    runs = [(["tests/" + name], name) for name in bad]
    short = good[:good.index(b"\n@", len(good) // 3) + 1]
    (cli_dir / "tests" / "fewer_2.fq").write_bytes(short)
    runs.append((["tests/reads_1.fq", "tests/fewer_2.fq"], "pair counts"))
    for args, what in runs:
        said = {}
        for by in ("1", "0"):
            r, _, how = run_map(cli_dir, args, ABM_CLI_DEVICE_PARSE=by)
            assert r.returncode != 0, what
            said[by] = (r.returncode, [ln for ln in r.stdout.splitlines() if "read" in ln or "batch" in ln])
            if by == "1":
                assert how and how["where"] == "device" and how["fallback_slices"] >= 1, (what, how)
        assert said["1"] == said["0"] and said["1"][1], (what, said)
