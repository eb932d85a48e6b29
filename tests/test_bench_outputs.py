"""bench.py's option handling and --dump-outputs writer, without a GPU."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def test_dump_outputs_files(tmp_path):
    """One .npy per record in f64 (the path sample in f32), path entries past path_len stored as -1
    whatever the buffer held there, the same rows on every call, and well under 64 MB at the
    headline's shape (4096 queries, path_cap 4096)."""
    import torch

    import bench

    n, cap = 4096, 4096
    rng = np.random.default_rng(5)
    plen = rng.integers(2, cap + 1, size=n).astype(np.int32)
    plen[:2] = (cap, 2)
    path = rng.integers(0, 1 << 20, size=(n, cap)).astype(np.int32)
    o = {"cost": torch.as_tensor(rng.random(n)), "plen": torch.as_tensor(plen), "path": torch.as_tensor(path),
         "nexp": torch.as_tensor(rng.integers(1, 1 << 19, size=n).astype(np.int32)),
         "status": torch.zeros(n, dtype=torch.int32)}
    bench.dump_outputs(str(tmp_path / "a"), o)
    o2 = dict(o, path=torch.as_tensor(np.where(np.arange(cap)[None, :] < plen[:, None], path, 7).astype(np.int32)))
    bench.dump_outputs(str(tmp_path / "b"), o2)  # other bytes in the unwritten tail: the same files
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["cost.npy", "n_expanded.npy", "path.npy", "path_len.npy", "path_rows.npy", "status.npy"]
    total = 0
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == (np.float32 if f == "path.npy" else np.float64), f
        assert np.array_equal(a, b), f
        total += a.nbytes
    assert total <= 64 * 10 ** 6
    rows = np.load(tmp_path / "a" / "path_rows.npy").astype(np.int64)
    assert len(rows) == bench.DUMP_PATH_ROWS and len(np.unique(rows)) == len(rows)
    got = np.load(tmp_path / "a" / "path.npy")
    want = np.where(np.arange(cap)[None, :] < plen[rows, None], path[rows], -1)
    assert np.array_equal(got.astype(np.int64), want)
    assert np.array_equal(np.load(tmp_path / "a" / "path_len.npy"), plen.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "cost.npy"), o["cost"].numpy())


def test_legs_need_full(monkeypatch, capsys):
    """The secondary legs moved behind --full: asking for one without it is an error, not a plain run."""
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--legs", "rrt"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and "--legs needs --full" in capsys.readouterr().err
