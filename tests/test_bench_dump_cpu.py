"""CPU suite: bench.py --dump-outputs writes float32 / float64 .npy files, ids exact, large arrays as a fixed seeded row sample."""
import os

import numpy as np
import torch

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
import bench


def test_dump_outputs_dtypes_and_values(tmp_path):
    D = torch.linspace(-1, 1, 100, dtype=torch.float32).reshape(10, 10)
    I = torch.arange(10 * 10, dtype=torch.int64).reshape(10, 10) * 9_999_991
    E = torch.randn((4096, 512), generator=torch.Generator().manual_seed(3))
    bench.dump_outputs(str(tmp_path / "out"), {"scores": D, "ids": I, "embeddings": E})
    assert sorted(os.listdir(tmp_path / "out")) == ["embeddings.npy", "ids.npy", "scores.npy"]
    s, i, e = (np.load(tmp_path / "out" / f"{n}.npy") for n in ("scores", "ids", "embeddings"))
    assert s.dtype == np.float32 and np.array_equal(s, D.numpy())
    assert i.dtype == np.float64 and np.array_equal(i.astype(np.int64), I.numpy())
    assert e.dtype == np.float32 and np.array_equal(e, E.numpy())      # 8 MB: written whole


def test_dump_outputs_samples_large_arrays_reproducibly(tmp_path):
    E = torch.randn((40_000, 512), generator=torch.Generator().manual_seed(4))   # 82 MB: above the per-array cap
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"embeddings": E})
    a, b = np.load(tmp_path / "a" / "embeddings.npy"), np.load(tmp_path / "b" / "embeddings.npy")
    rows = np.load(tmp_path / "a" / "embeddings_rows.npy")
    assert a.nbytes <= bench.DUMP_ARRAY_BYTES and len(a) == len(rows) > 0
    assert np.array_equal(a, b) and np.array_equal(rows, np.load(tmp_path / "b" / "embeddings_rows.npy"))
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, E.numpy()[rows.astype(np.int64)])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert 3 * total <= 64 << 20
