"""GPU: abm_ctx_reserve sizes every workspace the launches of a batch of that size ask for -- a reserved context maps
such a batch without growing a buffer (growing one frees the old allocation, and that waits for the whole device), and
gives what an unreserved context gives -- and a closed context returns the device memory of everything it allocated,
the sliced entry point's buffers included."""
import ctypes as C
import os

import pytest

from tests import synth

pytestmark = pytest.mark.gpu
FASTA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tRex1.fa")
N = 16384          # reads (pairs) per batch
L = 100            # bases per read
SLICES = 4         # of 4096 reads each
FIRST = [s * (N // SLICES) for s in range(SLICES + 1)]


@pytest.fixture(scope="module")
def pairs():
    """N pairs of 2 x L bases, every end exactly L bases long (synth.mutated_pairs cuts a few ends short: those pairs are
    left out)"""
    r1, r2 = synth.mutated_pairs(FASTA, N + N // 8, L, seed=23)
    keep = [(a, b) for a, b in zip(r1, r2) if len(a) == L and len(b) == L][:N]
    assert len(keep) == N
    return [a for a, _ in keep], [b for _, b in keep]


@pytest.fixture(scope="module")
def index(trex_index):
    import abismal_amd as A
    ix = A.Index(trex_index)
    yield ix
    ix.close()


def _same_bytes(got, want):
    if isinstance(want, tuple):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            _same_bytes(g, w)
    else:
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _regrowth_lines(capfd, traced_sections):
    err = capfd.readouterr().err
    if traced_sections:  # (the single-end entry points trace their sections: the variable did reach the library)
        assert "[abm host]" in err, "ABM_TRACE_HOST=1 printed nothing: the check below would be empty"
    return [ln for ln in err.splitlines() if "buffer regrown" in ln]


def test_reserved_single_end_context_grows_no_buffer(index, pairs, monkeypatch, capfd):
    import abismal_amd as A
    reads = pairs[0]
    plain = A.Context(index, 0)
    try:
        want = plain.map_se_sliced(reads, FIRST)[:3]
    finally:
        plain.close()
    monkeypatch.setenv("ABM_TRACE_HOST", "1")
    capfd.readouterr()
    ctx = A.Context(index, 0)
    try:
        ctx.reserve(N, L, paired=False)
        got = ctx.map_se_sliced(reads, FIRST)[:3]
    finally:
        ctx.close()
    lines = _regrowth_lines(capfd, True)
    print("\n".join(lines) if lines else "no buffer regrown")
    assert not lines, lines
    _same_bytes(got, want)


def test_reserved_paired_end_context_grows_no_buffer(index, pairs, monkeypatch, capfd):
    import abismal_amd as A
    plain = A.Context(index, 0)
    try:
        want = plain.map_pe(pairs[0], pairs[1])
    finally:
        plain.close()
    monkeypatch.setenv("ABM_TRACE_HOST", "1")
    capfd.readouterr()
    ctx = A.Context(index, 0)
    try:
        ctx.reserve(N, L, paired=True)
        got = ctx.map_pe(pairs[0], pairs[1])
    finally:
        ctx.close()
    lines = _regrowth_lines(capfd, False)
    print("\n".join(lines) if lines else "no buffer regrown")
    assert not lines, lines
    _same_bytes(got, want)


def _device_free_bytes():
    import abismal_amd as A
    lib = A.load_library()
    lib.abm_device_memory.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    free_b, total_b = C.c_uint64(), C.c_uint64()
    assert lib.abm_device_memory(0, C.byref(free_b), C.byref(total_b)) == 0
    return int(free_b.value)


def test_closed_contexts_return_their_sliced_buffers(index, pairs):
    """32 contexts in a row, each mapping the same 4-slice batch and then closed: the device's free memory after the last
    close is what it was after the first, to within one batch's sliced buffers.  (A context that does not free them
    loses that much -- rounded up to whole pages per buffer -- with every context.)"""
    import abismal_amd as A
    reads = pairs[0]
    # the device buffers only a sliced launch allocates: slice numbers per read (u16), reads each slice waits for, slice
    # boundaries, and the ordering kernels' histogram of (SLICES + 1) * 33 + 33 + SLICES + 2 words
    bound = N * 2 + SLICES * 4 + (SLICES + 1) * 4 + ((SLICES + 1) * 33 + 33 + SLICES + 2) * 4
    free_after = []
    for _ in range(32):
        ctx = A.Context(index, 0)
        try:
            ctx.map_se_sliced(reads, FIRST)
        finally:
            ctx.close()
        free_after.append(_device_free_bytes())
    print(f"free after the first close {free_after[0]}, after the last {free_after[-1]}, bound {bound}")
    assert abs(free_after[0] - free_after[-1]) <= bound, free_after
