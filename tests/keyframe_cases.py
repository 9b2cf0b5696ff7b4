"""Shared by the CPU and GPU suites of ivr_amd/keyframes.py: the seeded inputs, and the reference's code
(filter_research_update.py, with imagehash.phash behind its :97-99) restated plainly around Pillow, scipy and sklearn.  imagehash is
not installed here, so `imagehash_phash` below is what parity is pinned against: its phash() is convert('L'), a Lanczos resize to
32x32, scipy.fftpack.dct over both axes, the low 8x8 block against its median."""
import numpy as np
import scipy.fftpack
from PIL import Image
from sklearn.cluster import DBSCAN
from sklearn.metrics.pairwise import cosine_similarity

# rows 0..2 in front of the first offset, an empty segment [3,3), one-row segments [3,4) and [20,21), an empty [21,21), one segment of
# 1000 rows, and rows 1090.. past the last offset
SEGMENTS = np.array([3, 3, 4, 20, 21, 21, 1021, 1090], np.int64)
N_ROWS = 1100


# -- frames --------------------------------------------------------------------------------------------------------------------
def noise_frames(seed, n, h, w):
    return np.random.default_rng([seed, n, h, w, 0]).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def sinusoid_frames(seed, n, h, w):
    """Smooth frames: per channel a sum of three plane waves of random direction, a few periods across the frame."""
    rng = np.random.default_rng([seed, n, h, w, 1])
    y, x = np.mgrid[0:h, 0:w]
    y, x = y / max(h, 1), x / max(w, 1)
    out = np.zeros((n, h, w, 3))
    for i in range(n):
        for c in range(3):
            for _ in range(3):
                fy, fx, ph, amp = rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(0, 2 * np.pi), rng.uniform(10, 40)
                out[i, ..., c] += amp * np.sin(2 * np.pi * (fy * y + fx * x) + ph)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def low_contrast_frames(seed, n, h, w):
    """Gaussian noise of sigma 3 around a random grey level, drawn per cell of h // 64 x w // 64 pixels (per pixel up to 127 x 127) so
    that it survives the resize: per-pixel noise on a 1080p frame averages out to a constant 32 x 32 image."""
    rng = np.random.default_rng([seed, n, h, w, 2])
    base = rng.uniform(40, 215, (n, 1, 1, 1))
    ch, cw = max(1, h // 64), max(1, w // 64)
    g = rng.standard_normal((n, -(-h // ch), -(-w // cw), 3))
    g = np.repeat(np.repeat(g, ch, axis=1), cw, axis=2)[:, :h, :w]
    return np.clip(np.rint(base + 3.0 * g), 0, 255).astype(np.uint8)


FAMILIES = {"noise": noise_frames, "sinusoid": sinusoid_frames, "low_contrast": low_contrast_frames}


def mixed_frames(seed, n, h, w):
    """n frames, all different, cycling through the three families (the smooth one first)."""
    makers = [sinusoid_frames, noise_frames, low_contrast_frames]
    return np.concatenate([makers[i % 3](seed + i, 1, h, w) for i in range(n)])


# -- imagehash.phash restated --------------------------------------------------------------------------------------------------
def pillow_pixels(frame_rgb):
    """uint8 [32,32]: image.convert('L').resize((32, 32), LANCZOS)."""
    return np.asarray(Image.fromarray(np.ascontiguousarray(frame_rgb)).convert("L").resize((32, 32), Image.LANCZOS))


def imagehash_phash(frame_rgb):
    """(hash uint8 [8], coefficients float64 [8,8], median): imagehash.phash(img, hash_size=8, highfreq_factor=4); the hash is the bit
    array packed row-major, which is what str(ImageHash) prints in hex."""
    dct = scipy.fftpack.dct(scipy.fftpack.dct(pillow_pixels(frame_rgb), axis=0), axis=1)
    low = dct[:8, :8]
    med = np.median(low)
    return np.packbits(low > med), low, med


def pillow_resize(frames, size, mode, bilinear=False):
    """uint8 [n,size,size,3]: Image.resize per frame; stretch, or the long edge to `size` centred on a zero canvas (letterbox)."""
    flt = Image.BILINEAR if bilinear else Image.BICUBIC
    out = np.zeros((len(frames), size, size, 3), np.uint8)
    for i, f in enumerate(frames):
        h, w, _ = f.shape
        if mode == "stretch":
            out[i] = np.asarray(Image.fromarray(f).resize((size, size), flt))
        elif mode == "shortest_edge_crop":                          # the short edge to `size`, then the centre size x size
            rh, rw = (int(size * h / w), size) if w <= h else (size, int(size * w / h))
            oy, ox = (rh - size) // 2, (rw - size) // 2
            out[i] = np.asarray(Image.fromarray(f).resize((rw, rh), flt))[oy:oy + size, ox:ox + size]
        else:
            rh, rw = (size, max(1, int(size * w / h))) if h >= w else (max(1, int(size * h / w)), size)
            oy, ox = (size - rh) // 2, (size - rw) // 2
            out[i, oy:oy + rh, ox:ox + rw] = np.asarray(Image.fromarray(f).resize((rw, rh), flt))
    return out


# -- hashes and embeddings that drift ------------------------------------------------------------------------------------------
def hash_walk(n, seed, fresh=0.12, pool=40):
    """uint8 [n,8]: every hash is one of the last `pool` base hashes with 0 to 4 random bits flipped (two copies of a base differ in 8
    bits at most, mostly in 5 or fewer); the base is the previous row's half of the time, now and then a fresh random one.  So a row
    is often a duplicate of a kept row far back, and the size of the window decides."""
    rng = np.random.default_rng([seed, n, 3])
    bases, last = [rng.integers(0, 2, 64, dtype=np.uint8)], 0
    bits = np.zeros((n, 64), np.uint8)
    for i in range(n):
        r = rng.random()
        if r < fresh:
            bases.append(rng.integers(0, 2, 64, dtype=np.uint8))
            bases, last = bases[-pool:], min(len(bases), pool) - 1
        elif r < 0.5:
            last = int(rng.integers(0, len(bases)))
        cur = bases[last].copy()
        cur[rng.choice(64, int(rng.integers(0, 5)), replace=False)] ^= 1
        bits[i] = cur
    return np.packbits(bits, axis=1)


def embedding_walk(n, d, seed, fresh=0.12, pool=40):
    """float32 [n,d] of any norm: every row is one of the last `pool` anchor directions plus noise of relative size 0.05 to 0.25
    (cosine to the anchor 0.97 to 0.999, between two copies of an anchor 0.94 to 0.998: mostly above the threshold 0.95, sometimes
    below; between anchors about 0); the anchor is the previous row's half of the time, now and then a fresh one.  So a row often
    resembles a kept row far back, and the size of the window decides."""
    rng = np.random.default_rng([seed, n, d, 4])
    anchors, last = [rng.standard_normal(d)], 0
    rows = []
    for _ in range(n):
        r = rng.random()
        if r < fresh:
            anchors.append(rng.standard_normal(d))
            anchors, last = anchors[-pool:], min(len(anchors), pool) - 1
        elif r < 0.5:
            last = int(rng.integers(0, len(anchors)))
        a = anchors[last] / np.linalg.norm(anchors[last])
        x = a + rng.uniform(0.05, 0.25) * rng.standard_normal(d) / np.sqrt(d)
        rows.append(x * rng.uniform(0.5, 3.0))
    return np.asarray(rows, np.float32)


def video_embeddings(lengths, d, seed):
    """float32 [sum(lengths), d] of any norm, one video after the other: scenes of 5 to 40 frames from fresh random starts (cosine
    about 0 across a cut); inside a scene small turns (0.03 to 0.12 rad: one DBSCAN cluster at eps 0.05) and, one step in five, a
    turn of 0.5 to 0.7 rad (cosine 0.76 to 0.88: the same scene at 0.7, another cluster)."""
    rng = np.random.default_rng([seed, d, 5])
    rows = []
    for n in lengths:
        left = 0
        for _ in range(n):
            if left == 0:
                left = int(rng.integers(5, 41))
                x = rng.standard_normal(d)
            else:
                u = rng.standard_normal(d)
                u -= (u @ x) * x
                th = rng.uniform(0.5, 0.7) if rng.random() < 0.2 else rng.uniform(0.03, 0.12)
                x = np.cos(th) * x + np.sin(th) * u / np.linalg.norm(u)
            x /= np.linalg.norm(x)
            left -= 1
            rows.append(x * rng.uniform(0.5, 3.0))
    return np.asarray(rows, np.float32)


# -- the reference's loops restated --------------------------------------------------------------------------------------------
def _runs(n, seg_off):
    if seg_off is None:
        return [(0, n)]
    off = np.clip(np.asarray(seg_off, np.int64), 0, n)
    return [(int(a), int(max(a, b))) for a, b in zip(off[:-1], off[1:])]


def reference_hash_filter(hashes, seg_off=None, threshold=5, window=10):
    """filter_research_update.py:157-162 and :289-298 per segment, on 64-bit integers: keep uint8 [n]."""
    vals = [int.from_bytes(bytes(h), "big") for h in np.asarray(hashes, np.uint8)]
    keep = np.zeros(len(vals), np.uint8)
    for lo, hi in _runs(len(vals), seg_off):
        hash_window = []
        for i in range(lo, hi):
            duplicate = False
            for prev in hash_window:
                if bin(vals[i] ^ prev).count("1") <= threshold:
                    duplicate = True
                    break
            if not duplicate:
                keep[i] = 1
                hash_window.append(vals[i])
                if len(hash_window) > window:
                    hash_window.pop(0)
    return keep


def reference_window_filter(emb, seg_off=None, threshold=0.95, window=10):
    """filter_research_update.py:316-338 per segment in float64: (keep uint8 [n], the smallest |cosine - threshold| over every
    comparison the loop could make, whole window, no early exit)."""
    emb = np.asarray(emb, np.float64)
    keep = np.zeros(len(emb), np.uint8)
    margin = np.inf
    for lo, hi in _runs(len(emb), seg_off):
        embedding_window = []
        for i in range(lo, hi):
            is_unique = True
            if embedding_window:
                sims = cosine_similarity([emb[i]], emb[embedding_window])[0]
                margin = min(margin, float(np.abs(sims - threshold).min()))
                is_unique = not (sims >= threshold).any()
            if is_unique:
                keep[i] = 1
                embedding_window.append(i)
                if len(embedding_window) > window:
                    embedding_window.pop(0)
    return keep, margin


def reference_select_keyframes(emb, hashes, video_off, scene_threshold=0.7, hash_threshold=5, window=10, eps=0.05, min_samples=2,
                               sim_threshold=0.95):
    """Phases 2-4 of extract_advanced_keyframes_optimized (:274-338) per video, in float64 around sklearn: (rows, scene ids, margins),
    margins = the smallest distance of a scene cosine to scene_threshold, of a DBSCAN distance to eps, the smallest gap between the
    best two cosines of a group to its mean, and of a final-filter cosine to sim_threshold."""
    emb = np.asarray(emb, np.float64)
    m = {"scene": np.inf, "eps": np.inf, "winner": np.inf, "final": np.inf}
    rows_out, scenes_out = [], []
    for v0, v1 in zip(video_off[:-1], video_off[1:]):
        e, h = emb[v0:v1], hashes[v0:v1]
        if not len(e):
            continue
        bounds = [0]
        for i in range(1, len(e)):
            sim = cosine_similarity([e[i]], [e[i - 1]])[0][0]
            m["scene"] = min(m["scene"], abs(sim - scene_threshold))
            if sim < scene_threshold:
                bounds.append(i)
        bounds.append(len(e))
        selected = []
        for s0, s1 in zip(bounds[:-1], bounds[1:]):
            unique = s0 + np.flatnonzero(reference_hash_filter(h[s0:s1], None, hash_threshold, window))
            if not len(unique):
                continue
            if len(unique) < 2:
                clusters = [[0]]
            else:
                D = np.maximum(1.0 - cosine_similarity(e[unique]), 0.0)
                m["eps"] = min(m["eps"], float(np.abs(D[np.triu_indices(len(D), 1)] - eps).min()))
                labels = DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(D).labels_
                clusters = {}
                for idx, label in enumerate(labels):
                    clusters.setdefault(int(label), []).append(idx)
                clusters = list(clusters.values())
            for c in clusters:                                      # `cluster[0] != -1` never fires: the noise list counts too
                if len(c) == 1:
                    selected.append(int(unique[c[0]]))
                    continue
                sims = cosine_similarity(e[unique[c]], [e[unique[c]].mean(axis=0)])[:, 0]
                top = np.sort(sims)
                m["winner"] = min(m["winner"], float(top[-1] - top[-2]))
                selected.append(int(unique[c[int(np.argmax(sims))]]))
        selected.sort()
        keep, margin = reference_window_filter(e[selected], None, sim_threshold, window)
        m["final"] = min(m["final"], margin)
        for r in np.asarray(selected)[keep.astype(bool)]:
            rows_out.append(v0 + int(r))
            scenes_out.append(int(np.searchsorted(bounds[:-1], r, side="right") - 1))
    return np.asarray(rows_out, np.int64), np.asarray(scenes_out, np.int64), m
