"""GPU suite: compat.UnifiedIndex.incremental_update (unified_index.py:415-478) and UnifiedBuilderIntegration.incremental_update_fast.

The clip_processor is a duck-typed stand-in whose embedding of a file is drawn from an RNG seeded by the file's bytes, so a row does
not depend on the batch it was encoded in and an incrementally updated index can be compared exactly with a full rebuild of the final
directory: the same (file_path, similarity_score) pairs for every query."""
import hashlib
import json
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 64


class BytesSeededProcessor:
    """encode_images with the reference's signature (core.py:1556); counts its calls."""

    def __init__(self):
        self.calls = []

    def encode_images(self, image_paths, batch_size=32, validate_files=True, show_progress=True):
        self.calls.append(list(image_paths))
        out = np.empty((len(image_paths), D), np.float32)
        for i, p in enumerate(image_paths):
            seed = int.from_bytes(hashlib.sha256(open(p, "rb").read()).digest()[:8], "little")
            out[i] = np.random.default_rng(seed).standard_normal(D)
        return out


def _jpeg(path, seed):
    from PIL import Image
    px = np.random.default_rng(seed).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    Image.fromarray(px).save(path, quality=90)


def _make_dir(root):
    """40 small JPEGs in three folders."""
    n = 0
    for folder, count in (("video_a", 14), ("video_b", 13), ("video_c", 13)):
        os.makedirs(root / folder)
        for i in range(count):
            _jpeg(root / folder / f"{i:03d}.jpg", n)
            n += 1
    return root


def _queries():
    return np.random.default_rng(123).standard_normal((5, D)).astype(np.float32)


def _hits(ui, k=10):
    return [[(r["metadata"]["file_path"], r["similarity_score"]) for r in ui.search_vectors(q, k=k)] for q in _queries()]


def _built(tmp_path, name="index.npz"):
    from ivr_amd.compat import UnifiedIndex
    root = _make_dir(tmp_path / "keyframes")
    proc = BytesSeededProcessor()
    ui = UnifiedIndex()
    ui.create_unified_index(str(root), proc, str(tmp_path / name))
    assert ui.faiss_index.ntotal == 40
    return ui, proc, root


def _small_change(root):
    """delete 2 files, overwrite 1 with other pixels, add 1: 2 new or modified out of 39, inside the default threshold 0.1"""
    os.remove(root / "video_a" / "003.jpg")
    os.remove(root / "video_c" / "012.jpg")
    _jpeg(root / "video_b" / "005.jpg", 1005)
    _jpeg(root / "video_a" / "100.jpg", 1100)


def _consistent(ui, n):
    assert ui.faiss_index.ntotal == n and len(ui.metadata_list) == n
    assert [m["vector_index"] for m in ui.metadata_list] == list(range(n))
    assert ui.vectors.shape == (n, D)
    assert sorted(ui.file_hashes) == sorted(os.path.relpath(m["file_path"], os.path.dirname(os.path.dirname(m["file_path"])))
                                            for m in ui.metadata_list)


def test_update_equals_full_rebuild(tmp_path):
    from ivr_amd.compat import UnifiedIndex
    ui, proc, root = _built(tmp_path)
    assert ui.vectors.shape == (40, D)                      # cached: the update must drop it
    _small_change(root)
    proc.calls.clear()
    stats = ui.incremental_update(str(root), proc, "")
    assert (stats["scanned_files"], stats["new_files"], stats["modified_files"], stats["deleted_files"]) == (39, 1, 1, 2)
    assert stats["rebuild_required"] is False and stats["update_time"] > 0
    assert len(proc.calls) == 1 and len(proc.calls[0]) == 2         # one batched call, only the changed files
    _consistent(ui, 39)
    assert ui.metadata_list[-1]["file_path"] == str(root / "video_a" / "100.jpg")       # new rows are appended
    rebuilt = UnifiedIndex()
    rebuilt.create_unified_index(str(root), BytesSeededProcessor(), str(tmp_path / "rebuilt.npz"))
    got, want = _hits(ui), _hits(rebuilt)
    assert all(len(h) == 10 for h in want)
    assert got == want
    # a second call finds nothing to do
    proc.calls.clear()
    again = ui.incremental_update(str(root), proc, "")
    assert (again["scanned_files"], again["new_files"], again["modified_files"], again["deleted_files"]) == (39, 0, 0, 0)
    assert again["rebuild_required"] is False and proc.calls == []
    assert _hits(ui) == want


def test_deletions_alone_are_applied(tmp_path):
    from ivr_amd.compat import UnifiedIndex
    ui, proc, root = _built(tmp_path)
    os.remove(root / "video_b" / "000.jpg")
    proc.calls.clear()
    stats = ui.incremental_update(str(root), proc, "")
    assert (stats["new_files"], stats["modified_files"], stats["deleted_files"]) == (0, 0, 1) and proc.calls == []
    _consistent(ui, 39)
    rebuilt = UnifiedIndex()
    rebuilt.create_unified_index(str(root), BytesSeededProcessor(), str(tmp_path / "rebuilt.npz"))
    assert _hits(ui) == _hits(rebuilt)


def test_many_changes_ask_for_a_rebuild(tmp_path):
    ui, proc, root = _built(tmp_path)
    before = _hits(ui)
    for i in range(8):                                      # 8 of 40 = 20 % > 0.1
        _jpeg(root / "video_c" / f"{i:03d}.jpg", 2000 + i)
    proc.calls.clear()
    stats = ui.incremental_update(str(root), proc, "")
    assert stats["rebuild_required"] is True and stats["modified_files"] == 8
    assert proc.calls == [] and _hits(ui) == before
    _consistent(ui, 40)
    # the threshold comes from config.incremental_threshold when there is one
    ui.config = types.SimpleNamespace(incremental_threshold=0.25)
    stats = ui.incremental_update(str(root), proc, "")
    assert stats["rebuild_required"] is False and stats["modified_files"] == 8
    assert _hits(ui) != before


def test_index_file_round_trip(tmp_path):
    from ivr_amd.compat import UnifiedIndex, load_optimized_index
    ui, proc, root = _built(tmp_path)
    npz = str(tmp_path / "index.npz")
    ui.close()
    ui = UnifiedIndex()                                     # nothing loaded: incremental_update loads index_file first
    _small_change(root)
    stats = ui.incremental_update(str(root), proc, npz)
    assert (stats["new_files"], stats["modified_files"], stats["deleted_files"]) == (1, 1, 2)
    loaded = load_optimized_index(npz)
    assert loaded.file_hashes == ui.file_hashes and len(loaded.file_hashes) == 39
    _consistent(loaded, 39)
    assert loaded.metadata_list == ui.metadata_list
    assert _hits(loaded) == _hits(ui)
    again = loaded.incremental_update(str(root), proc, npz)
    assert (again["new_files"], again["modified_files"], again["deleted_files"], again["rebuild_required"]) == (0, 0, 0, False)


def test_file_without_hashes_asks_for_a_rebuild(tmp_path):
    from ivr_amd.compat import UnifiedIndex
    ui, proc, root = _built(tmp_path)
    old = str(tmp_path / "old.npz")
    as_bytes = lambda obj: np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)
    np.savez(old, vectors=ui.vectors, metadata=as_bytes(ui.metadata_list), csv_mappings=as_bytes({}))
    legacy = UnifiedIndex()
    stats = legacy.incremental_update(str(root), proc, old)
    assert legacy.file_hashes == {}
    assert stats["rebuild_required"] is True and stats["new_files"] == 40
    assert legacy.faiss_index.ntotal == 40


def test_empty_directory_raises(tmp_path):
    ui, proc, root = _built(tmp_path)
    empty = tmp_path / "empty"
    os.makedirs(empty)
    with pytest.raises(ValueError, match="no .jpg files"):
        ui.incremental_update(str(empty), proc, "")
    assert ui.faiss_index.ntotal == 40


def test_builder_forwards(tmp_path):
    from ivr_amd.compat import UnifiedBuilderIntegration
    ui, proc, root = _built(tmp_path)
    builder = UnifiedBuilderIntegration(types.SimpleNamespace(clip_processor=proc))
    with pytest.raises(ValueError, match="not loaded"):
        builder.incremental_update_fast(str(root))
    assert builder.load_unified_index_fast(str(tmp_path / "index.npz"))
    stamp = os.stat(tmp_path / "index.npz").st_mtime_ns
    _small_change(root)
    stats = builder.incremental_update_fast(str(root))
    assert (stats["new_files"], stats["modified_files"], stats["deleted_files"], stats["rebuild_required"]) == (1, 1, 2, False)
    _consistent(builder.unified_index, 39)
    assert os.stat(tmp_path / "index.npz").st_mtime_ns == stamp         # "" as the index file: in memory only, nothing rewritten
