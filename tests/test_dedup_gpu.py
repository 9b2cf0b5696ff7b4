"""GPU parity: the device-side keep/drop chain vs the oracle of video_frame_filter.py:63-70."""
import ctypes as C

import numpy as np
import pytest
import torch

import reduce_cases as RC
from oracle import search_ref as S

pytestmark = pytest.mark.gpu


def _gpu_mask(E, thr, batches):
    from ivr_amd.dedup import DedupState
    st = DedupState(E.shape[1])
    out = []
    for a, b in batches:
        out.append(st.keep_mask(torch.from_numpy(E[a:b]).cuda(), thr).cpu().numpy())
    return np.concatenate(out).astype(bool)


def test_golden_sequence(golden):
    g = golden("search")
    E = g["dedup_emb"]
    assert np.array_equal(_gpu_mask(E, 0.98, [(0, 64)]), g["dedup_keep"])
    # the chain continues across batch boundaries through the carried state
    assert np.array_equal(_gpu_mask(E, 0.98, [(0, 1), (1, 30), (30, 31), (31, 64)]), g["dedup_keep"])


@pytest.mark.parametrize("d,thr", [(384, 0.98), (512, 0.9), (768, 0.995)])
def test_random_walk(d, thr):
    # deterministic seed search: skip sequences with a decision inside float32 noise of the threshold
    for seed in range(d, d + 50):
        rng = np.random.default_rng(seed)
        E = (np.cumsum(rng.standard_normal((500, d)) * 0.2, axis=0) + 2.0).astype(np.float32)
        sims, prev = [], None
        for e in E:
            if prev is not None:
                sims.append(S.cosine_1x1(e, prev))
            if prev is None or sims[-1] < thr:
                prev = e
        if np.abs(np.array(sims) - thr).min() > 2e-5:
            break
    else:
        pytest.fail("no well-separated sequence found")
    ref = S.dedup_keep_mask(E, thr)
    assert np.array_equal(_gpu_mask(E, thr, [(0, 200), (200, 500)]), ref)
    assert 1 < ref.sum() < 500


# -- the chain against oracle/reduce_ref.py: every instantiation of dedup_kernel, margins derived from the cosine bound -------------
@pytest.mark.parametrize("d,thr", RC.WALK_CASES)
def test_random_walk_with_derived_margin(d, thr):
    """PER = 6, 16 and 32, partly filled last registers, d = 2048 in chunks of 4 rows; one batch, (0, 1) + (1, n) and splits at rows
    that are no multiple of the chunk length.  Every decision clears the threshold by four times the bound of its cosine."""
    print(f"\nd={d} thr={thr}: {RC.check_random_walk(RC.Gpu, d, thr)} of 300 frames kept")


def test_small_chain_at_every_split_point():
    """d = 2048, n = 9 (chunks of 4), frames kept as the last row of a chunk; every split 0 .. 9 gives the unsplit mask and leaves
    (1, last kept row) in the state after each batch."""
    RC.check_small_chain_splits(RC.Gpu)


def test_a_batch_that_keeps_nothing_leaves_the_state_alone():
    RC.check_carried_state(RC.Gpu)


def test_zero_rows_in_the_chain():
    RC.check_zero_rows(RC.Gpu)


@pytest.mark.parametrize("d", RC.TIE_D)
def test_cosine_exactly_at_the_threshold_is_dropped(d):
    """sim = 1.0 and 0.5 exactly: dropped at thr = sim (>=), kept at the next float32 above it."""
    RC.check_exact_ties(RC.Gpu, d)


def test_rows_wider_than_2048_are_refused():
    from ivr_amd import filters as F
    from ivr_amd.dedup import DedupState
    E = np.ones((3, 2049), np.float32)
    st = DedupState(2049)
    with pytest.raises(ValueError, match="2048"):
        st.keep_mask(torch.from_numpy(E).cuda(), 0.98)
    assert not st.state.cpu().numpy().any()
    with pytest.raises(ValueError, match="2048"):
        F.filter_similar_frames_in_scene(E, [0, 1, 2], {"enable_similarity_filtering": True, "similarity_threshold": 0.9, "min_frame_distance": 1})
