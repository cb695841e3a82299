"""CPU: bench.py's --dump-outputs helpers -- hits split into their fields, CIGARs resolved from their slots or the
long-CIGAR arena, a sample that is the same from run to run, float32 / float64 files only, and the 64 MB limit."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_hits_split_into_fields(bench):
    w0 = np.array([(0x0100 << 16) | 3, (0 << 16) | 0xFFFF], dtype=np.uint32)  # flags 0x100 diffs 3; flags 0 diffs -1
    pos = np.array([3_100_000_000, 0], dtype=np.uint32)
    hits = np.stack([w0, pos], 1).view(np.int32)
    d = bench.dump_hits("x_", hits)
    assert d["x_pos"].dtype == np.float64 and d["x_pos"].tolist() == [3_100_000_000, 0]
    assert d["x_diffs"].dtype == np.float32 and d["x_diffs"].tolist() == [3, -1]
    assert d["x_flags"].tolist() == [0x100, 0]


def test_cigars_from_slots_and_arena(bench):
    stride = 4
    slots = np.zeros((3, stride), dtype=np.uint32)
    slots[0, :2] = [100 << 4, 5 << 4 | 1]
    slots[1, 0] = 2  # a long CIGAR: its ops start at arena[2]
    arena = np.array([9, 9, 11, 12, 13, 14, 15, 9], dtype=np.uint32)
    cig_n = np.array([2, 5, 0], dtype=np.uint32)
    d = bench.dump_cigars("", slots.view(np.int32), cig_n.view(np.int32), arena, stride)
    assert d["cigar_offsets"].tolist() == [0, 2, 7, 7]
    assert d["cigar_ops"].tolist() == [100 << 4, 5 << 4 | 1, 11, 12, 13, 14, 15]
    cig_n[1] = 7  # beyond the arena
    with pytest.raises(RuntimeError):
        bench.dump_cigars("", slots.view(np.int32), cig_n.view(np.int32), arena, stride)


def test_sample_fixed_and_bounded(bench):
    assert bench.dump_sample_ids(10).tolist() == list(range(10))
    a, b = bench.dump_sample_ids(10_000_000), bench.dump_sample_ids(10_000_000)
    assert len(a) == bench.DUMP_SAMPLE and np.array_equal(a, b)
    assert (np.diff(a) > 0).all() and a[-1] < 10_000_000


def test_write_dump(bench, tmp_path):
    bench.write_dump(str(tmp_path / "out"), {"a": np.arange(4, dtype=np.float32), "b": np.zeros(2)})
    assert np.load(tmp_path / "out" / "a.npy").tolist() == [0, 1, 2, 3]
    assert np.load(tmp_path / "out" / "b.npy").dtype == np.float64
    with pytest.raises(RuntimeError):
        bench.write_dump(str(tmp_path / "big"), {"a": np.zeros(bench.DUMP_MAX_BYTES // 8 + 1)})
    assert not (tmp_path / "big").exists()
