"""Shared by the CPU and GPU suites of the neighbour graph: the float64 cosine matrix the reference sorts (core.py:3513-3526), its
brute-force top-k of the OTHER rows, and the rule under which a float32 ranking must agree with it."""
import numpy as np

from oracle.reduce_ref import flat_score_bound

TOP, THRESHOLD = 10, 0.7                 # core.py:3522-3524


def cosines64(X):
    """float64 [m,m]: rows normalised in float64 (a zero norm counts as 1), then X X^T, as oracle.search_ref.similarity_graph."""
    f = np.asarray(X, np.float64)
    n = np.linalg.norm(f, axis=1, keepdims=True)
    n[n == 0] = 1
    f = f / n
    return f @ f.T


def brute_force64(sim, k, threshold):
    """Per row the at most k best other rows with sim > threshold (None: any), best first: a list of int lists."""
    out = []
    for j in range(len(sim)):
        order = [i for i in np.argsort(-sim[j], kind="stable").tolist() if i != j][:k]
        out.append([i for i in order if threshold is None or sim[j, i] > threshold])
    return out


def clear_rows(sim, k, threshold, d):
    """bool [m]: the rows whose float32 ranking must equal the float64 one.  The float64 scores of the row's best k + 1 others and
    its own (the reference finds the row itself by its place in the order) differ pairwise by more than 2 flat_score_bound(d, 1), so
    two float32 scores, each within the bound of its float64 value, keep their order; and none of them lies within the bound of the
    threshold, so each falls on the same side of it."""
    b = float(flat_score_bound(d, 1.0))
    clear = np.zeros(len(sim), bool)
    for j in range(len(sim)):
        s = np.sort(sim[j])[::-1][:k + 2]                # sim[j, j] is among them: nothing exceeds a cosine of 1 by more than rounding
        gaps_ok = len(s) < 2 or float(np.min(-np.diff(s))) > 2 * b
        thr_ok = threshold is None or float(np.min(np.abs(s - threshold))) > b
        clear[j] = gaps_ok and thr_ok
    return clear
