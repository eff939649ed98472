"""bench.py's command line, host side only: --full is off by default and --dump-outputs writes the
rows it is handed as float32, whole below its size cap and as a fixed seeded sample of rows above it."""
import os
import sys

import numpy as np
import torch

import bench


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, "", 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    rows = torch.arange(40 * 8, dtype=torch.float32).reshape(40, 8) / 7.0
    d = str(tmp_path / "whole")
    bench.dump_outputs(d, rows)
    assert os.listdir(d) == ["probs.npy"]
    y = np.load(os.path.join(d, "probs.npy"))
    assert y.dtype == np.float32
    np.testing.assert_array_equal(y, rows.numpy())

    # 10 rows of 32 bytes + the header room fit under this cap
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096 + 10 * 32)
    got = []
    for name in ("s1", "s2"):
        d = str(tmp_path / name)
        bench.dump_outputs(d, rows)
        assert os.path.getsize(os.path.join(d, "probs.npy")) <= bench.DUMP_MAX_BYTES
        got.append(np.load(os.path.join(d, "probs.npy")))
    np.testing.assert_array_equal(got[0], got[1])  # the same rows from run to run
    assert got[0].shape == (10, 8)
    idx = (got[0][:, 0] * 7.0 / 8.0).round().astype(int)  # row r starts at 8 r / 7
    assert (np.diff(idx) > 0).all()  # in batch order, no row twice
    np.testing.assert_array_equal(got[0], rows.numpy()[idx])
