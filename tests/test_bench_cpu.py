"""CPU tests of bench.py's --dump-outputs writer: the files a run leaves for comparing two builds output for output."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_small_surface(tmp_path):
    V, N = torch.randn(10, 3), torch.randn(10, 3)
    T = torch.randint(0, 10, (7, 3), dtype=torch.int32)
    bench.dump_outputs(str(tmp_path), V, N, T)
    assert np.load(tmp_path / "counts.npy").tolist() == [10.0, 7.0]
    assert np.load(tmp_path / "V.npy").dtype == np.float32 and np.array_equal(np.load(tmp_path / "V.npy"), V.numpy())
    assert np.array_equal(np.load(tmp_path / "N.npy"), N.numpy())
    t = np.load(tmp_path / "T.npy")
    assert t.dtype == np.float64 and np.array_equal(t, T.numpy())


def test_dump_outputs_large_surface_is_a_fixed_sample_under_64_mb(tmp_path):
    nV, nT = 3 * bench.DUMP_ROWS + 5, 6 * bench.DUMP_ROWS + 1
    g = torch.Generator().manual_seed(1)
    V, N = torch.randn(nV, 3, generator=g), torch.randn(nV, 3, generator=g)
    T = torch.randint(0, nV, (nT, 3), dtype=torch.int32, generator=g)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), V, N, T)
    total = 0
    for name in ("counts", "V", "N", "T"):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert np.array_equal(a, b), name
        total += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert total <= 64e6
    assert np.load(tmp_path / "a" / "counts.npy").tolist() == [nV, nT]
    rows = np.sort(np.random.default_rng(0).choice(nT, bench.DUMP_ROWS, replace=False))
    assert np.array_equal(np.load(tmp_path / "a" / "T.npy"), T.numpy()[rows].astype(np.float64))
    rows = np.sort(np.random.default_rng(0).choice(nV, bench.DUMP_ROWS, replace=False))
    assert np.array_equal(np.load(tmp_path / "a" / "V.npy"), V.numpy()[rows]) and np.array_equal(np.load(tmp_path / "a" / "N.npy"), N.numpy()[rows])


def test_bench_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout
