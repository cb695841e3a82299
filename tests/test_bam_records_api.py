"""BAM pieces from the kernels, without a GPU: the entry point that asks for them is declared, exported and checks its
arguments; the Python binding reaches it; and tests/bam_format.py -- the yardstick of the GPU tests -- restates the
CLI's own put_bam_record byte for byte (a -virtual-gpus run, once as SAM and once as BAM)."""
import ctypes as C
import inspect
import os
import subprocess

from tests import bam_format

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "abismal_amd", "abismal-amd")


def test_header_declares_the_record_format():
    h = open(os.path.join(ROOT, "include", "abismal_amd.h")).read()
    assert "enum { ABM_RECORDS_SAM = 0, ABM_RECORDS_BAM = 1 };" in h
    assert "int abm_ctx_set_record_format(abm_ctx *ctx, int format);" in h
    import abismal_amd.api as api
    assert "abm_ctx_set_record_format" in api.EXPORTED_SYMBOLS
    assert (api.RECORDS_SAM, api.RECORDS_BAM) == (0, 1)


def test_library_exports_it_and_checks_its_arguments():
    import abismal_amd as A
    lib = A.load_library()
    f = lib.abm_ctx_set_record_format
    f.argtypes = [C.c_void_p, C.c_int]
    f.restype = C.c_int
    lib.abm_last_error.restype = C.c_char_p
    assert f(None, 1) < 0
    assert b"null" in lib.abm_last_error()
    # (an unknown format, likewise refused with a text; with a context it is refused before anything is set)
    assert f(None, 7) < 0 and lib.abm_last_error()


def test_python_context_reaches_it():
    import abismal_amd as A
    sig = inspect.signature(A.Context.set_record_format)
    assert "bam" in sig.parameters and sig.parameters["bam"].default is False
    sig = inspect.signature(A.Context.map_se_sliced)
    assert "tails" in sig.parameters and sig.parameters["tails"].default is False


def test_piece_and_assemble_restate_the_clis_bam_records(oracle, trex_index, tmp_path):
    """every record of a BAM run equals assemble(name, piece(fields of the same run's SAM line))"""
    fq = str(tmp_path / "r")
    oracle.simulate(os.path.join(ROOT, "tests", "golden", "tRex1.fa"), fq, 3000, single_end=True, seed=33)
    for extra, out in (([], "o.sam"), (["-B"], "o.bam")):
        r = subprocess.run([CLI, "map", "-virtual-gpus", "1", "-t", "2", "-i", trex_index, "-o", str(tmp_path / out)] + extra + [fq + "_1.fq"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    _, names, recs = bam_format.records_of_stream(bam_format.bgzf_decompress(open(tmp_path / "o.bam", "rb").read()))
    refids = {n: i for i, n in enumerate(names)}
    lines = [ln for ln in open(tmp_path / "o.sam", "rb") if not ln.startswith(b"@")]
    assert len(lines) == len(recs) and len(recs) > 2000
    strands = set()
    for ln, rec in zip(lines, recs):
        name, tail = ln.split(b"\t", 1)
        strands.add(int(tail.split(b"\t")[0]) & 0x10)
        assert bam_format.assemble(name, bam_format.piece_from_tail(b"\t" + tail, refids)) == rec, ln
    assert strands == {0, 0x10}
