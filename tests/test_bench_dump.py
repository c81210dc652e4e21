"""bench.py --dump-outputs (CPU): what dump_outputs writes for small and for large arrays, and the plain / --full
split of the command line."""
import sys

import numpy as np
import torch

import bench


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    small = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7)
    # channels-last storage: the dump is in logical NCHW order whatever the strides
    big = torch.arange(2 * 8 * 9 * 11, dtype=torch.float64).reshape(2, 8, 9, 11).contiguous(
        memory_format=torch.channels_last)
    bench.dump_outputs(str(tmp_path / "a"), {"small": small, "big": big})
    bench.dump_outputs(str(tmp_path / "b"), {"small": small, "big": big})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (2, 3, 5, 7) and np.array_equal(s, small.numpy())
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float32 and b.shape == (1000,)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, big.numel(), 1000))
    assert np.array_equal(b, idx.astype(np.float32))  # big's logical flat element i holds the value i
    assert len(np.unique(idx)) > 500  # a spread sample, not one element repeated
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))  # same elements from run to run


def test_dump_budget():
    """Two arrays of at most DUMP_MAX_ELEMS float32 elements stay below 64 MB."""
    assert 2 * bench.DUMP_MAX_ELEMS * 4 <= 64 * 10**6


def test_full_and_dump_options_default_off(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 4 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"
