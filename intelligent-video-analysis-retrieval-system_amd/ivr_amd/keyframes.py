"""Perceptual hashing and the look-back duplicate filters of the research keyframe extractor, on the GPU.

Stands in for what `AdvancedKeyframeExtractor` (`filter_research_update.py`) runs before and after the clustering of `cluster.py`:
`imagehash.phash` of every frame (`:97-99`, `:250`), the perceptual-duplicate filter inside a scene (`:157-162`, `:289-298`) and the
final temporal filter over the chosen representatives (`:316-338`); `select_keyframes` is its phases 2-4 for a batch of videos.

Definitions (the `_ref` functions below are these in numpy + Pillow):

  hash      per frame uint8 [h,w,3]: grey = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 (Pillow's convert('L')); resized to 32x32 by
            Pillow's 8-bit resampler with the Lanczos filter; the float64 type-II DCT of it, unnormalised, columns then rows, low 8x8
            block: with C[k][m] = cos(pi k (2m+1) / 64) (the library's table, ivr_phash_cos_table), A[k][x] = 2 sum_y C[k][y] p[y][x]
            and B[k][l] = 2 sum_x A[k][x] C[l][x], both sums ascending, every product and sum rounded on its own; bit[k][l] =
            B[k][l] > (s[31] + s[32]) / 2 over the sorted values s; packed row-major, most significant bit first (np.packbits), so
            hash.tobytes().hex() is str(imagehash.phash(img)).  The one departure: on a constant frame every coefficient but B[0][0]
            is rounding residue, here of the direct sums and in the reference of its FFT, so those 63 bits follow this definition
            and not the reference
  segments  seg_off (int64 [nseg+1], ascending, empty runs allowed), as in clip search and DBSCAN; rows outside every segment get 0;
            None: all rows are one segment
  window    both filters walk a segment in row order and hold the last `window` KEPT rows of it (1 <= window <= 64): a kept row is
            appended, then the oldest leaves once there are more than `window`.  hash_keep_mask keeps row i iff no hash h in the
            window has popcount(h_i xor h) <= threshold; kept_window_mask keeps it iff no row j in the window has cos(e_i, e_j) >=
            threshold, the cosine with the arithmetic of ivr_rowwise_cosine (cluster._cosine32), so numpy reproduces every decision
"""
import ctypes

import numpy as np
import torch

from . import _ffi, _staging, cluster
from .index import FlatIPIndex

SIM_THRESHOLD = 0.95         # filter_research_update.py: SIM_THRESHOLD
SCENE_THRESHOLD = 0.7        # SCENE_THRESHOLD
PERCEPTUAL_THRESHOLD = 5     # PERCEPTUAL_THRESHOLD
TEMPORAL_WINDOW = 10         # TEMPORAL_WINDOW
FRAME_SIZE = (224, 224)      # FRAME_SIZE


# -- the definitions in numpy --------------------------------------------------------------------------------------------------
def cos_table():
    """C float64 [8,32], C[k][m] = cos(pi k (2m+1) / 64): the 256 doubles the kernel multiplies with, from the library (no GPU)."""
    buf = (ctypes.c_double * 256)()
    _ffi.call("ivr_phash_cos_table", buf)
    return np.frombuffer(buf, np.float64).reshape(8, 32).copy()


def _check_frames(frames, what):
    if not isinstance(frames, (np.ndarray, torch.Tensor)) or frames.ndim != 4 or frames.shape[3] != 3 or \
            frames.dtype not in (np.uint8, torch.uint8):
        raise ValueError(f"{what}: frames must be uint8 [n,h,w,3]")
    n, h, w, _ = frames.shape
    if n and not (1 <= h <= _ffi.IVR_PHASH_MAX_SIDE and 1 <= w <= _ffi.IVR_PHASH_MAX_SIDE):
        raise ValueError(f"{what}: h={h} w={w} outside [1,{_ffi.IVR_PHASH_MAX_SIDE}]")
    return n, h, w


def phash_ref(frames, bgr=False, return_pixels=False):
    """frames uint8 [n,h,w,3] -> hashes uint8 [n,8] (and the 32x32 grey images uint8 [n,32,32]): the definition of the module
    docstring, the resize by Pillow itself."""
    from PIL import Image
    frames = np.asarray(frames)
    n, h, w = _check_frames(frames, "phash_ref")
    C = cos_table()
    hashes, pixels = np.zeros((n, 8), np.uint8), np.zeros((n, 32, 32), np.uint8)
    for i in range(n):
        f = frames[i].astype(np.uint32)
        r, b = (f[..., 2], f[..., 0]) if bgr else (f[..., 0], f[..., 2])
        grey = ((r * 19595 + f[..., 1] * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)
        px = np.asarray(Image.fromarray(grey, "L").resize((32, 32), Image.LANCZOS))
        pixels[i] = px
        p = px.astype(np.float64)
        A = np.zeros((8, 32))
        for y in range(32):                                         # ascending y, product and sum rounded one by one
            A = A + C[:, y:y + 1] * p[y:y + 1, :]
        A = 2.0 * A
        B = np.zeros((8, 8))
        for x in range(32):
            B = B + A[:, x:x + 1] * C[:, x][None, :]
        B = 2.0 * B
        s = np.sort(B.ravel())
        hashes[i] = np.packbits(B > (s[31] + s[32]) / 2)
    return (hashes, pixels) if return_pixels else hashes


def _check_window(threshold, window, what, integer):
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)):
        raise ValueError(f"{what}: window must be an integer, got {type(window).__name__}")
    if not 1 <= window <= _ffi.IVR_KEEPWIN_MAX_WINDOW:
        raise ValueError(f"{what}: window={window} outside [1,{_ffi.IVR_KEEPWIN_MAX_WINDOW}]")
    if integer:
        if isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)):
            raise ValueError(f"{what}: threshold must be an integer, got {type(threshold).__name__}")
        return int(min(max(threshold, -1), 65)), int(window)        # below 0 nothing is near, above 64 everything
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or threshold != threshold:
        raise ValueError(f"{what}: threshold must be a number that is not NaN, got {threshold!r}")
    return float(np.float32(threshold)), int(window)


def _runs(n, seg_off):
    if seg_off is None:
        return [(0, n)]
    off = np.clip(np.asarray(seg_off).astype(np.int64).reshape(-1), 0, n)
    return [(int(a), int(max(a, b))) for a, b in zip(off[:-1], off[1:])]


def hash_keep_mask_ref(hashes, seg_off=None, threshold=PERCEPTUAL_THRESHOLD, window=TEMPORAL_WINDOW):
    """hashes uint8 [n,8] -> keep uint8 [n]: the definition of the module docstring."""
    hashes = np.ascontiguousarray(np.asarray(hashes, np.uint8)).reshape(-1, 8)
    threshold, window = _check_window(threshold, window, "hash_keep_mask_ref", True)
    bits = np.unpackbits(hashes, axis=1)
    keep = np.zeros(len(hashes), np.uint8)
    for lo, hi in _runs(len(hashes), seg_off):
        win = []
        for i in range(lo, hi):
            if not any(int((bits[i] != bits[j]).sum()) <= threshold for j in win):
                keep[i] = 1
                win.append(i)
                if len(win) > window:
                    win.pop(0)
    return keep


def kept_window_mask_ref(emb, seg_off=None, threshold=SIM_THRESHOLD, window=TEMPORAL_WINDOW):
    """emb float32 [n,d] -> keep uint8 [n]: the definition of the module docstring, the cosines by cluster._cosine32."""
    emb = np.ascontiguousarray(np.asarray(emb, np.float32))
    threshold, window = _check_window(threshold, window, "kept_window_mask_ref", False)
    keep = np.zeros(len(emb), np.uint8)
    for lo, hi in _runs(len(emb), seg_off):
        win = []
        for i in range(lo, hi):
            cos = cluster._cosine32(np.broadcast_to(emb[i], (len(win), emb.shape[1])), emb[win]) if win else np.zeros(0, np.float32)
            if not (cos >= np.float32(threshold)).any():
                keep[i] = 1
                win.append(i)
                if len(win) > window:
                    win.pop(0)
    return keep


# -- the library calls ---------------------------------------------------------------------------------------------------------
def _dev_frames(frames, what):
    from .preprocess import _frames_on_device
    _check_frames(frames, what)
    return _frames_on_device(frames)


def phash_device(frames, bgr=False, return_pixels=False):
    """The perceptual hash of every frame on the device: frames uint8 [n,h,w,3] (numpy or CUDA tensor) -> hashes uint8 CUDA [n,8], with
    return_pixels also the 32x32 grey images uint8 CUDA [n,32,32] the hash was taken from.  No host synchronisation."""
    t = _dev_frames(frames, "phash")
    n, h, w, _ = t.shape
    hashes = torch.empty((n, 8), dtype=torch.uint8, device=t.device)
    pixels = torch.empty((n, 32, 32), dtype=torch.uint8, device=t.device) if return_pixels else None
    _ffi.call("ivr_phash", _ffi.CTX, t, n, h, w, _ffi.PP_BGR if bgr else 0, hashes, pixels, device=t.device)
    return (hashes, pixels) if return_pixels else hashes


def phash(frames, bgr=False, return_pixels=False):
    """phash_device as numpy arrays."""
    out = phash_device(frames, bgr, return_pixels)
    return tuple(t.cpu().numpy() for t in out) if return_pixels else out.cpu().numpy()


def hash_keep_mask_device(hashes, seg_off=None, threshold=PERCEPTUAL_THRESHOLD, window=TEMPORAL_WINDOW):
    """The perceptual-duplicate filter on the device: hashes uint8 [n,8] -> keep uint8 CUDA [n].  No host synchronisation unless
    hashes or seg_off had to be staged."""
    threshold, window = _check_window(threshold, window, "hash_keep_mask", True)
    dev = hashes.device if isinstance(hashes, torch.Tensor) and hashes.is_cuda else torch.device("cuda", torch.cuda.current_device())
    h = _staging.dev_u8(hashes, 8, dev, "hash_keep_mask")
    seg, staged, nseg = _staging.segments(seg_off, dev, "hash_keep_mask")
    keep = torch.empty(max(len(h), 1), dtype=torch.uint8, device=dev)
    _ffi.call("ivr_hash_keep_mask", _ffi.CTX, h, len(h), seg, nseg, threshold, window, keep, device=dev)
    _staging.sync_if_staged(staged or _staging.is_staged(h, hashes), dev)
    return keep[:len(h)]


def hash_keep_mask(hashes, seg_off=None, threshold=PERCEPTUAL_THRESHOLD, window=TEMPORAL_WINDOW):
    """hash_keep_mask_device as a numpy array."""
    return hash_keep_mask_device(hashes, seg_off, threshold, window).cpu().numpy()


def kept_window_mask_device(emb, seg_off=None, threshold=SIM_THRESHOLD, window=TEMPORAL_WINDOW):
    """The look-back similarity filter on the device: emb float32 [n,d] -> keep uint8 CUDA [n].  No host synchronisation unless emb or
    seg_off had to be staged."""
    threshold, window = _check_window(threshold, window, "kept_window_mask", False)
    if not isinstance(emb, (np.ndarray, torch.Tensor)) or emb.ndim != 2 or emb.shape[1] < 1:
        raise ValueError(f"kept_window_mask: emb must be [n,d], got {tuple(getattr(emb, 'shape', ()))}")
    dev = emb.device if isinstance(emb, torch.Tensor) and emb.is_cuda else torch.device("cuda", torch.cuda.current_device())
    e = _staging.dev_f32(emb, dev)
    seg, staged, nseg = _staging.segments(seg_off, dev, "kept_window_mask")
    keep = torch.empty(max(len(e), 1), dtype=torch.uint8, device=dev)
    _ffi.call("ivr_kept_window_mask", _ffi.CTX, e, len(e), e.shape[1], seg, nseg, threshold, window, keep, device=dev)
    _staging.sync_if_staged(staged or _staging.is_staged(e, emb), dev)
    return keep[:len(e)]


def kept_window_mask(emb, seg_off=None, threshold=SIM_THRESHOLD, window=TEMPORAL_WINDOW):
    """kept_window_mask_device as a numpy array."""
    return kept_window_mask_device(emb, seg_off, threshold, window).cpu().numpy()


# -- phases 2-4 of extract_advanced_keyframes_optimized ------------------------------------------------------------------------
def _video_offsets(video_off, n, what):
    if video_off is None:
        return np.array([0, n], np.int64)
    off = np.asarray(video_off)
    if not np.issubdtype(off.dtype, np.integer) or off.ndim != 1 or len(off) < 2:
        raise ValueError(f"{what}: video_off must be integers [nvideos+1]")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError(f"{what}: video_off must ascend from 0 to {n}, got {off.tolist()}")
    return off


def _scene_ids(rows, scene_off, video_off):
    """The number of row r's scene inside its video: scene_off holds the starts of the non-empty scenes (every video start among them)."""
    scene = np.searchsorted(scene_off, rows, side="right") - 1
    video = np.searchsorted(video_off, rows, side="right") - 1
    return scene - np.searchsorted(scene_off, video_off[video], side="left")


def select_keyframes_ref(embeddings, hashes, video_off=None, scene_threshold=SCENE_THRESHOLD, hash_threshold=PERCEPTUAL_THRESHOLD,
                         window=TEMPORAL_WINDOW, eps=cluster.CLUSTER_EPS, min_samples=cluster.MIN_CLUSTER_SIZE,
                         sim_threshold=SIM_THRESHOLD):
    """select_keyframes in numpy, composed from the refs of its steps; the DBSCAN scores are the float32 products of the rows
    normalised in float32 (the device's differ in the last bits: a distance within the flat index's score bound of eps may fall
    either way)."""
    X = np.ascontiguousarray(np.asarray(embeddings, np.float32))
    n = len(X)
    video_off = _video_offsets(video_off, n, "select_keyframes_ref")
    cut = np.zeros(n + 1, bool)
    if n > 1:
        cut[1:n] = cluster._cosine32(X[:-1], X[1:]) < np.float32(scene_threshold)
    cut[video_off] = True
    scene_off = np.flatnonzero(cut)
    keep = hash_keep_mask_ref(hashes, scene_off, hash_threshold, window)
    reps = []
    for lo, hi in zip(scene_off[:-1], scene_off[1:]):
        rows = lo + np.flatnonzero(keep[lo:hi])
        if not len(rows):
            continue
        raw = X[rows]
        nrm = np.sqrt((raw.astype(np.float32) ** 2).sum(1, dtype=np.float32))
        unit = (raw / np.where(nrm > 0, nrm, np.float32(1))[:, None]).astype(np.float32)
        labels, _, ncl = cluster.dbscan_ref(unit @ unit.T, eps, min_samples)
        groups = [np.flatnonzero(labels == c) for c in range(int(ncl[0]))] + [np.flatnonzero(labels < 0)]
        groups = [g for g in groups if len(g)]
        off = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
        reps.extend(rows[cluster.representatives_ref(raw, off, np.concatenate(groups))].tolist())
    reps = np.sort(np.asarray(reps, np.int64))
    final = reps[kept_window_mask_ref(X[reps], np.searchsorted(reps, video_off), sim_threshold, window).astype(bool)]
    return final, _scene_ids(final, scene_off, video_off)


def select_keyframes(embeddings, hashes, video_off=None, scene_threshold=SCENE_THRESHOLD, hash_threshold=PERCEPTUAL_THRESHOLD,
                     window=TEMPORAL_WINDOW, eps=cluster.CLUSTER_EPS, min_samples=cluster.MIN_CLUSTER_SIZE,
                     sim_threshold=SIM_THRESHOLD):
    """Phases 2-4 of extract_advanced_keyframes_optimized (filter_research_update.py:274-338) for a batch of videos in one call.
    embeddings float32 [n,d] and hashes uint8 [n,8] of the frames in decode order, video v = the rows video_off[v] : video_off[v+1]
    (host integers from 0 to n; None: one video) -> (rows int64 [m], scene_ids int64 [m]) numpy arrays: the kept frames in row order
    and the number of each one's scene inside its video (the reference's CSV columns original_frame_idx and scene_id).

      scenes           a cut in front of row i where cos(e_i, e_{i-1}) < scene_threshold (ivr_rowwise_cosine), and at every video start
      duplicates       hash_keep_mask per scene
      clustering       the survivors, compacted, go into a temporary FlatIPIndex (normalised) with the scene offsets recomputed; dbscan
                       per scene
      representatives  one per cluster and one for the noise rows of a scene taken together (the reference's `cluster[0] != -1` tests
                       a frame position, so it never fires; cluster_similar_frames keeps the same quirk): the row closest to the
                       group's mean, taken over the embeddings as they came (select_representatives over a second, unnormalised index)
      final filter     the representatives in row order through kept_window_mask per video
    """
    if not isinstance(embeddings, (np.ndarray, torch.Tensor)) or embeddings.ndim != 2:
        raise ValueError(f"select_keyframes: embeddings must be [n,d], got {tuple(getattr(embeddings, 'shape', ()))}")
    n, d = embeddings.shape
    video_off = _video_offsets(video_off, n, "select_keyframes")
    if len(hashes) != n:
        raise ValueError(f"select_keyframes: {len(hashes)} hashes for {n} embeddings")
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    dev = embeddings.device if isinstance(embeddings, torch.Tensor) and embeddings.is_cuda else \
        torch.device("cuda", torch.cuda.current_device())
    X = _staging.dev_f32(embeddings, dev)
    H = _staging.dev_u8(hashes, 8, dev, "select_keyframes")
    voff = torch.from_numpy(video_off).to(dev)
    cut = torch.zeros(n + 1, dtype=torch.bool, device=dev)
    if n > 1:
        sims = torch.empty(n - 1, dtype=torch.float32, device=dev)
        _ffi.call("ivr_rowwise_cosine", _ffi.CTX, X[:-1], X[1:], n - 1, d, sims, device=dev)
        cut[1:n] = sims < np.float32(scene_threshold)
    cut[voff] = True
    scene_off = torch.nonzero(cut).reshape(-1)                      # the starts of the non-empty scenes, and n
    keep = hash_keep_mask_device(H, scene_off, hash_threshold, window)
    survivors = torch.nonzero(keep).reshape(-1)
    before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(keep.to(torch.int64), 0)])
    off2 = before[scene_off].contiguous()                           # the scenes over the compacted rows
    unit, raw = FlatIPIndex(d, device=dev.index), FlatIPIndex(d, device=dev.index)
    try:
        rows = X[survivors].contiguous()
        unit.add(rows, normalize=True)
        raw.add(rows)
        labels, _, ncl = cluster.dbscan_device(unit, eps, min_samples, off2)
        # the noise rows of a scene form one more group, numbered after the scene's clusters (an empty group gives no representative)
        scene = torch.searchsorted(off2, torch.arange(len(survivors), device=dev), right=True) - 1
        labels = torch.where(labels < 0, ncl[scene], labels)
        group_off, members = cluster.cluster_members(labels, ncl + 1, off2)
        reps = cluster.select_representatives(raw, group_off, members)
    finally:
        unit.close()
        raw.close()
    reps = survivors[torch.sort(reps[reps >= 0]).values]
    keep2 = kept_window_mask_device(X[reps].contiguous(), torch.searchsorted(reps, voff), sim_threshold, window)
    final = reps[keep2.bool()].cpu().numpy()
    return final, _scene_ids(final, scene_off.cpu().numpy(), video_off)


# -- the reference's class -----------------------------------------------------------------------------------------------------
class PerceptualHash:
    """What extract_perceptual_hash returns: the 8 hash bytes; a - b is the Hamming distance, str() the 16 hex digits, as with
    imagehash.ImageHash."""
    __slots__ = ("bytes",)

    def __init__(self, b):
        self.bytes = bytes(b) if isinstance(b, (bytes, bytearray)) else np.asarray(b, np.uint8).tobytes()
        if len(self.bytes) != 8:
            raise ValueError(f"PerceptualHash: 8 bytes expected, got {len(self.bytes)}")

    def __sub__(self, other):
        return bin(int.from_bytes(self.bytes, "big") ^ int.from_bytes(other.bytes, "big")).count("1")

    def __eq__(self, other):
        return isinstance(other, PerceptualHash) and self.bytes == other.bytes

    def __hash__(self):
        return hash(self.bytes)

    def __str__(self):
        return self.bytes.hex()

    __repr__ = __str__


class AdvancedKeyframeExtractor:
    """filter_research_update.py:78 with the reference's method names.  The embeddings come from the FrameFilter handed in (the
    reference loads facebook/dino-vits16 by name at import time); hashes, filters and clustering run on the GPU."""

    def __init__(self, frame_filter=None):
        self.frame_filter = frame_filter

    def _filter(self):
        if self.frame_filter is None:
            raise RuntimeError("AdvancedKeyframeExtractor: no FrameFilter - pass frame_filter=FrameFilter(weights=...)")
        return self.frame_filter

    def extract_embedding(self, image):
        """:89-95."""
        return self._filter().extract_embedding(image)

    def extract_perceptual_hash(self, image):
        """:97-99: a PIL image or a uint8 RGB array [h,w,3] -> PerceptualHash."""
        a = np.array(image.convert("RGB") if hasattr(image, "convert") else image)        # a copy: a PIL image's array is read-only
        return PerceptualHash(phash(a[None])[0])

    def detect_scene_changes(self, embeddings, threshold=SCENE_THRESHOLD):
        """:101-111: [0, the rows whose cosine to their predecessor is below threshold ..., n]."""
        from .filters import calculate_similarities
        sims = calculate_similarities(np.asarray(embeddings, np.float32)) if len(embeddings) > 1 else []
        return [0] + [i + 1 for i, s in enumerate(sims) if s < threshold] + [len(embeddings)]

    def cluster_similar_frames(self, embeddings, frame_indices=None):
        """:113-134."""
        return cluster.cluster_similar_frames(embeddings, frame_indices)

    def select_representative_frame(self, cluster_indices, embeddings, frame_info=None):
        """:136-155."""
        return cluster.select_representative_frame(cluster_indices, embeddings, frame_info)

    def is_duplicate_by_hash(self, current_hash, hash_window):
        """:157-162."""
        return any(abs(current_hash - prev) <= PERCEPTUAL_THRESHOLD for prev in hash_window)

    def extract_advanced_keyframes(self, frames_bgr, pts_time=None):
        """extract_advanced_keyframes_optimized (:225-369) over decoded frames, without its file I/O: frames_bgr uint8 [n,h,w,3] in
        cv2 order, pts_time the n timestamps (ascending; None: left out) -> the rows of the reference's CSV as dicts with n, pts_time,
        original_frame_idx and scene_id.  Every frame is stretched to 224x224 once (:246); that image is embedded and hashed."""
        from .preprocess import resize_frames_u8
        ff = self._filter()
        frames = _dev_frames(np.asarray(frames_bgr) if not isinstance(frames_bgr, torch.Tensor) else frames_bgr, "extract_advanced_keyframes")
        n = len(frames)
        if pts_time is not None and (len(pts_time) != n or (np.diff(np.asarray(pts_time, np.float64)) < 0).any()):
            raise ValueError("extract_advanced_keyframes: pts_time must hold one ascending timestamp per frame")
        if n == 0:
            return []
        small = resize_frames_u8(frames, "stretch", FRAME_SIZE[0])
        hashes = phash_device(small, bgr=True)
        emb = ff.tower.encode_frames(small, "identity", ff.mean, ff.std, bgr=True, normalize=False)
        rows, scenes = select_keyframes(emb, hashes)
        return [{"n": i, "pts_time": None if pts_time is None else round(float(pts_time[r]), 3), "original_frame_idx": int(r),
                 "scene_id": int(s)} for i, (r, s) in enumerate(zip(rows, scenes))]
