"""Shared by the CPU and GPU suites of the frame clustering: the seeded inputs, the reference's two functions
(filter_research_update.py:113-155) restated literally in float64 around sklearn, and the conditions under which a float32 clustering
must agree with them."""
from collections import defaultdict

import numpy as np
from sklearn.cluster import DBSCAN
from sklearn.metrics.pairwise import cosine_similarity

from oracle.reduce_ref import flat_score_bound

NS = (2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 700)      # tile, LDS-block and workgroup boundaries, one size with several column blocks
DS = (20, 512)
MIN_SAMPLES = (1, 2, 3, 5)
EPS = 0.05                                                  # the reference's CLUSTER_EPS
# boundaries at 15 / 16 / 17 and 64 / 65, an empty segment [17, 17), segments of one row ([15, 16), [16, 17), [64, 65)), row 0 in front
# of the first offset and rows 90 .. 99 past the last: the offsets of test_temporal_gpu.test_segments
SEGMENTS = np.array([1, 15, 16, 17, 17, 19, 64, 65, 90], np.int64)


def unit32(x):
    """Rows divided by their norm in float64, rounded to float32 once."""
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def drifting_chains(n, d, seed=0, lengths=(1, 13)):
    """n unit rows [n,d] in permuted order: chains of 1 to 12 rows in which every row is its predecessor turned by 0.05 to 0.3 rad
    towards a fresh random direction (1 - cos between neighbours 0.001 to 0.045, two steps apart mostly beyond 0.05), every chain
    from a fresh random start.  A chain of one row is noise, the ends of a chain are border rows once min_samples asks for two
    neighbours, and long slow stretches are dense enough for min_samples = 5."""
    rng = np.random.default_rng([seed, n, d])
    rows = []
    while len(rows) < n:
        x = rng.standard_normal(d)
        x /= np.linalg.norm(x)
        for _ in range(int(rng.integers(*lengths))):
            rows.append(x)
            u = rng.standard_normal(d)
            u -= (u @ x) * x
            u /= np.linalg.norm(u)
            th = rng.uniform(0.05, 0.3)
            x = np.cos(th) * x + np.sin(th) * u
            x /= np.linalg.norm(x)
    return unit32(np.array(rows[:n])[rng.permutation(n)])


def one_chain(n, d, seed=0, theta=0.25, back=8):
    """n unit rows in chain order in which every row reaches only its predecessor and its successor at eps = 0.05: each step turns
    the row by theta towards a direction orthogonal to the last `back` rows, so the cosine k <= back steps apart is cos(theta)^k
    (0.969, 0.939, ...), and rows further apart are as good as unrelated."""
    rng = np.random.default_rng([seed, n, d, 1])
    x = rng.standard_normal(d)
    x /= np.linalg.norm(x)
    rows = [x]
    while len(rows) < n:
        u = rng.standard_normal(d)
        P = np.array(rows[-back:]).T
        u -= P @ np.linalg.lstsq(P, u, rcond=None)[0]      # the part of u orthogonal to the span of the recent rows
        u /= np.linalg.norm(u)
        x = np.cos(theta) * rows[-1] + np.sin(theta) * u
        rows.append(x / np.linalg.norm(x))
    return unit32(np.array(rows))


def contested_border(d=20, seed=0):
    """Nine unit rows on a circle: clumps of four at -0.50 .. -0.30 rad and 0.30 .. 0.50 rad, and row 4 at 0 between them, which
    reaches (1 - cos 0.30 = 0.0447 <= 0.05) exactly one row of each clump and nothing else (1 - cos 0.40 = 0.079).  With
    min_samples = 4 the clumps are two clusters of core rows and row 4 is a border row both clusters claim."""
    rng = np.random.default_rng([seed, d, 2])
    q, _ = np.linalg.qr(rng.standard_normal((d, 2)))
    ang = np.array([-0.50, -0.45, -0.40, -0.30, 0.0, 0.30, 0.40, 0.45, 0.50])
    return unit32(np.cos(ang)[:, None] * q[:, 0] + np.sin(ang)[:, None] * q[:, 1])


def distances64(X):
    """The reference's distance matrix in float64: 1 - cosine_similarity, negative rounding residue clipped (sklearn refuses it)."""
    return np.maximum(1.0 - cosine_similarity(np.asarray(X, np.float64)), 0.0)


def snapped_eps(D, nominal, d):
    """(eps, margin): the middle of the widest gap between consecutive pair distances (and the window's ends) within +-20 % of
    `nominal`, and half that gap: no pair distance lies within `margin` of eps."""
    lo, hi = 0.8 * nominal, 1.2 * nominal
    v = D[np.triu_indices(len(D), 1)]
    v = np.sort(np.concatenate([[lo, hi], v[(v > lo) & (v < hi)]]))
    i = int(np.argmax(np.diff(v)))
    return float(0.5 * (v[i] + v[i + 1])), float(0.5 * (v[i + 1] - v[i]))


def sklearn_dbscan(D, eps, min_samples):
    """(labels int32, core uint8, nclusters int32 [1]) of sklearn's DBSCAN on the precomputed distances."""
    fit = DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(D)
    core = np.zeros(len(D), np.uint8)
    core[fit.core_sample_indices_] = 1
    return fit.labels_.astype(np.int32), core, np.array([fit.labels_.max() + 1], np.int32)


def reference_cluster_similar_frames(embeddings, eps=EPS, min_samples=2):
    """filter_research_update.py:113-134."""
    if len(embeddings) < 2:
        return [[0]] if len(embeddings) else []
    clustering = DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(distances64(embeddings))
    clusters = defaultdict(list)
    for idx, label in enumerate(clustering.labels_):
        clusters[int(label)].append(idx)
    return list(clusters.values())


def reference_representative(cluster_indices, embeddings, gaps=None):
    """filter_research_update.py:136-155 in float64; gaps collects best cosine - second best cosine of the cluster."""
    if len(cluster_indices) == 1:
        return cluster_indices[0]
    embeddings = np.asarray(embeddings, np.float64)
    centroid = np.mean([embeddings[i] for i in cluster_indices], axis=0)
    best_idx, best_sim, sims = 0, -1, []
    for i, emb_idx in enumerate(cluster_indices):
        sim = cosine_similarity([embeddings[emb_idx]], [centroid])[0][0]
        sims.append(sim)
        if sim > best_sim:
            best_sim, best_idx = sim, i
    if gaps is not None:
        top = np.sort(sims)
        gaps.append(float(top[-1] - top[-2]))
    return cluster_indices[best_idx]


def clear_winner(gap, d):
    """The condition under which a float32 argmax must agree with the float64 one: the best two cosines of the cluster differ by
    more than the bound the flat index states for one float32 inner product of unit rows."""
    return gap > float(flat_score_bound(d, 1.0))


def border_and_noise(labels, core):
    return int(((core == 0) & (labels >= 0)).sum()), int((labels < 0).sum())
