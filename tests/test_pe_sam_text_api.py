"""The paired-end SAM-text entry point without a GPU: declared in the header, exported, argument checks, and its
Python face (Context.set_sam_tails, Context.map_pe(sam=...))."""
import ctypes as C
import inspect
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_pe_sam_tails():
    h = open(os.path.join(ROOT, "include", "abismal_amd.h")).read()
    assert "int abm_ctx_pe_sam_tails(abm_ctx *ctx, uint64_t lo, uint64_t hi, const char **tails, uint32_t *stride," in h
    import abismal_amd.api as api
    assert "abm_ctx_pe_sam_tails" in api.EXPORTED_SYMBOLS


def test_pe_sam_tails_rejects_null_arguments():
    import abismal_amd as A
    lib = A.load_library()
    f = lib.abm_ctx_pe_sam_tails
    f.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    tails, stride, lens, kinds = C.c_void_p(), C.c_uint32(), C.c_void_p(), C.c_void_p()
    assert f(None, 0, 0, C.byref(tails), C.byref(stride), C.byref(lens), C.byref(kinds)) != 0
    assert f(None, 0, 0, None, None, None, None) != 0
    lib.abm_ctx_set_sam_tails.argtypes = [C.c_void_p, C.c_int, C.c_int]
    assert lib.abm_ctx_set_sam_tails(None, 1, 0) != 0


def test_python_context_exposes_pe_text():
    import abismal_amd as A
    assert callable(getattr(A.Context, "set_sam_tails", None))
    sig = inspect.signature(A.Context.set_sam_tails)
    assert list(sig.parameters)[1:] == ["on", "allow_ambig"]
    sig = inspect.signature(A.Context.map_pe)
    assert "sam" in sig.parameters and sig.parameters["sam"].default is False
