"""What the two suites of the clip search share (test_temporal_cpu.py, test_temporal_gpu.py): the reference's TemporalAnalyzer loops
(core.py:3584-3739, 3812-3828) restated literally in float64 around sklearn's cosine_similarity, and the seeded inputs."""
import numpy as np
from sklearn.metrics.pairwise import cosine_similarity

D_FEAT = 16
MARGIN = 1e-4          # no float64 window mean may lie this close to the threshold, or float32 could decide differently


# -- the reference, restated literally in float64 ----------------------------------------------------------------------------------
def reference_sequence_similarity(seq1, seq2):                       # core.py:3812-3828
    if len(seq1) != len(seq2) or seq1.shape != seq2.shape:
        return 0.0
    frame_similarities = []
    for f1, f2 in zip(seq1, seq2):
        frame_similarities.append(cosine_similarity([f1], [f2])[0][0])
    return float(np.mean(frame_similarities))


def reference_find(target, database, L, threshold, all_means=None):      # core.py:3644-3702
    if len(target) < L or len(database) < L:
        return []
    out = []
    for target_start in range(len(target) - L + 1):
        target_seq = target[target_start:target_start + L]
        for db_start in range(len(database) - L + 1):
            db_seq = database[db_start:db_start + L]
            v = reference_sequence_similarity(target_seq, db_seq)
            if all_means is not None:
                all_means.append(v)
            if v >= threshold:
                out.append((db_start, v))
    out.sort(key=lambda x: x[1], reverse=True)
    return out


def reference_scene_boundaries(features, threshold=0.3, min_scene_length=5):      # core.py:3584-3642
    if len(features) < min_scene_length * 2:
        return [(0, len(features) - 1)]
    similarities = []
    for i in range(len(features) - 1):
        similarities.append(cosine_similarity([features[i]], [features[i + 1]])[0][0])
    boundaries = []
    current_start = 0
    for i, sim in enumerate(similarities):
        if sim < threshold:
            if i - current_start >= min_scene_length:
                boundaries.append((current_start, i))
                current_start = i + 1
    if current_start < len(features):
        boundaries.append((current_start, len(features) - 1))
    return boundaries


def reference_transition_frames(features, scene_boundaries):          # core.py:3704-3739
    transition_frames = []
    for i in range(len(scene_boundaries) - 1):
        _, current_end = scene_boundaries[i]
        next_start, _ = scene_boundaries[i + 1]
        for frame_idx in range(max(0, current_end - 2), min(len(features), next_start + 3)):
            if frame_idx not in transition_frames:
                transition_frames.append(frame_idx)
    return sorted(transition_frames)


# -- inputs ----------------------------------------------------------------------------------------------------------------------------
def clip_case(T, N, L, seed=20240):
    """T target frames and N database frames, float32 [.,16]: the database holds noisy copies of target runs, so that some windows
    score well above the threshold and most well below."""
    rng = np.random.default_rng([seed, T, N, L])
    target = rng.standard_normal((T, D_FEAT)).astype(np.float32)
    database = rng.standard_normal((N, D_FEAT)).astype(np.float32)
    for at in range(0, max(N - T + 1, 0), 17):
        database[at:at + T] = target + 0.35 * rng.standard_normal((T, D_FEAT)).astype(np.float32)
    return target, database


def as_result_list(lims, D, I):
    """The list find_similar_sequences builds from the range call: (target start, db start) order, then a stable sort by score."""
    out = [(int(s), float(w)) for s, w in zip(I, D)]
    out.sort(key=lambda x: x[1], reverse=True)
    return out
