"""The one numpy definition of the per-row segment bounds (ivr_amd/_staging.segment_bounds), which dbscan_ref, knn_graph_ref and
similarity_graphs read and which the segment-bounds kernel of the self-joins (csrc/self_join.hip) restates."""
import numpy as np

from cluster_cases import SEGMENTS
from ivr_amd._staging import segment_bounds

# what cluster._segment_starts returned for SEGMENTS = [1, 15, 16, 17, 17, 19, 64, 65, 90] and n = 100 before the two definitions
# became one: the start of the row's run, row + 1 for row 0 and for rows 90 .. 99
STARTS = [1] + [1] * 14 + [15, 16, 17, 17] + [19] * 45 + [64] + [65] * 25 + list(range(91, 101))
RUNS = [(1, 15), (15, 16), (16, 17), (17, 19), (19, 64), (64, 65), (65, 90)]


def test_rows_inside_a_run_get_its_bounds_and_all_others_an_empty_range():
    lo, hi = segment_bounds(100, SEGMENTS)
    assert lo.dtype == hi.dtype == np.int64 and lo.shape == hi.shape == (100,)
    assert lo.tolist() == STARTS
    inside = np.zeros(100, bool)
    for a, b in RUNS:
        assert (lo[a:b] == a).all() and (hi[a:b] == b).all()
        inside[a:b] = True
    outside = np.flatnonzero(~inside)
    assert outside.tolist() == [0] + list(range(90, 100))          # in front of seg_off[0] and behind seg_off[-1]
    assert (lo[outside] == outside + 1).all() and (hi[outside] == outside + 1).all()
    assert (np.diff(lo) >= 0).all() and ((lo <= np.arange(100)) == inside).all()


def test_runs_are_clipped_to_the_stored_rows():
    lo, hi = segment_bounds(70, SEGMENTS)
    assert lo.tolist() == STARTS[:70] and (hi[65:] == 70).all() and (hi[:65] == segment_bounds(100, SEGMENTS)[1][:65]).all()
    lo, hi = segment_bounds(6, np.array([-5, 3, 3, 4]))            # [-5, 3) from row 0 on, the empty run [3, 3), row 3, rows in no run
    assert lo.tolist() == [0, 0, 0, 3, 5, 6] and hi.tolist() == [3, 3, 3, 4, 5, 6]


def test_no_segments_is_one_run():
    lo, hi = segment_bounds(100, None)
    assert (lo == 0).all() and (hi == 100).all() and lo.dtype == hi.dtype == np.int64
    lo, hi = segment_bounds(0, SEGMENTS)
    assert lo.shape == hi.shape == (0,)
