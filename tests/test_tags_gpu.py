"""GPU suite of the zero-shot tagging (ivr_amd/tagging.py, csrc/tags.hip): D (to the bit), J and count of ivr_index_tag_rows for exact
equality with the numpy definition tag_rows_ref fed with the witness scores, that is the scores a temporary FlatIPIndex holding the
labels reports (rescore_device) for the reconstructed stored rows as queries; P and Z within tag_prob_bound of the float64 softmax of
those float32 scores (the largest observed ratio to the bound is printed); tag_segments for exact equality with tag_segments_ref fed
with the kernel's own P and J; a float64 argmax as a witness that does not go through our scores; the compat calls.

The bound is asserted with spread = 2: the rows and the labels are unit vectors, so every score lies in [-1, 1] up to rounding."""
import functools

import numpy as np
import pytest
import torch

from cluster_cases import NS, SEGMENTS, drifting_chains, unit32
from ivr_amd import _ffi, tagging
from ivr_amd.index import FlatIPIndex
from oracle.reduce_ref import flat_score_bound

pytestmark = pytest.mark.gpu

TMAX = _ffi.IVR_TAG_MAX_TOP
CS = (1, 15, 16, 17, 64, 65, 130, 1000)
TS = (1, 5, TMAX)
LOWEST = np.float32(-np.finfo(np.float32).max)
FLT_MIN = tagging.FLT_MIN
SPREAD = 2.0
NAMES = ("D", "P", "J", "count", "Z")


def labels_of(C, d):
    return unit32(np.random.default_rng([7, C, d]).standard_normal((C, d)))


def build(X, ids=None):
    index = FlatIPIndex(X.shape[1])
    if ids is None:
        index.add(X)
    else:
        index.add_with_ids(X, ids)
    return index


def witness(index, L, normalize=False):
    """S float32 [N,C]: what a FlatIPIndex holding the labels reports for (query = stored row j, stored row = label i)."""
    lab = FlatIPIndex(L.shape[1])
    lab.add(L, normalize=normalize)
    N, C = index.ntotal, len(L)
    rows = torch.from_numpy(index.reconstruct_n()).to(index.device)
    cand = torch.arange(C, dtype=torch.int64, device=index.device).repeat(N, 1).contiguous()
    S = lab.rescore_device(rows, cand)[0].cpu().numpy()
    lab.close()
    return S


@functools.lru_cache(maxsize=None)
def rows_case(N, d):
    X = drifting_chains(N, d)
    return build(X), X


@functools.lru_cache(maxsize=None)
def case(N, d, C):
    """(index, X, L, S) of one shape: built and scored once, shared by the tests below and left unchanged."""
    index, X = rows_case(N, d)
    L = labels_of(C, d)
    return index, X, L, witness(index, L)


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what="", names=NAMES):
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {name}: {g.dtype} {g.shape}, expected {w.dtype} {w.shape}"
        assert np.array_equal(bits(g), bits(w)), f"{what} {name} differ in rows {np.unique(np.nonzero(bits(g) != bits(w))[0])[:10]}"


def check(got, S, scale, t, min_prob=0.0, what="", spread=SPREAD):
    """D, J, count exactly the definition on the witness scores; P and Z within the bound of float64.  Returns the largest ratio of an
    observed error to what the bound allows."""
    D, P, J, count, Z = got
    Dr, Pr, Jr, cr, Zr = tagging.tag_rows_ref(S, scale, t, min_prob)
    same((D, J, count), (Dr, Jr, cr), what, ("D", "J", "count"))
    C = S.shape[1]
    bound = tagging.tag_prob_bound(C, scale, spread)
    P64, Z64 = tagging.softmax64(S + np.float32(0), scale)
    used = J >= 0
    want = np.take_along_axis(P64, np.where(used, J, 0), 1)
    rp = tagging.bound_ratio(P[used], want[used], bound, FLT_MIN)
    rz = tagging.bound_ratio(Z, Z64, bound)
    assert (P[~used] == 0).all()
    assert rp <= 1.0 and rz <= 1.0, f"{what}: |P - P64| reaches {rp:.3f} and |Z - Z64| {rz:.3f} of the bound {bound:.3e}"
    return max(rp, rz)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("d", (20, 512))
def test_every_shape_matches_the_definition(d, C):
    worst = 0.0
    for N in NS:
        index, X, L, S = case(N, d, C)
        for t in TS:
            got = tagging.tag_rows(index, L, t)
            worst = max(worst, check(got, S, 100.0, t, what=f"N={N} d={d} C={C} t={t}"))
            assert (got[3] == min(t, C)).all()
            if t > C:
                assert (got[2][:, C:] == -1).all() and (got[0][:, C:] == LOWEST).all()
    print(f"d={d} C={C}: largest |error| / bound = {worst:.4f} (bound {tagging.tag_prob_bound(C, 100.0, SPREAD):.3e})")


def test_the_limits_are_the_librarys():
    assert tagging.tag_max_top() == TMAX and tagging.tag_max_labels() == _ffi.IVR_TAG_MAX_LABELS


def test_repeated_calls_and_a_second_stream_give_the_same_bits():
    index, X, L, S = case(700, 512, 130)
    lab = torch.from_numpy(L).to(index.device)
    first = [o.clone() for o in tagging.tag_rows_device(index, lab, 5)]
    again = tagging.tag_rows_device(index, lab, 5)
    side = torch.cuda.Stream(device=index.device)
    side.wait_stream(torch.cuda.current_stream(index.device))
    with torch.cuda.stream(side):
        other = tagging.tag_rows_device(index, lab, 5)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b, c in zip(first[1::3], again[1::3], other[1::3]):                          # P and Z: the same BITS, not merely equal values
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert [o.dtype for o in first] == [torch.float32, torch.float32, torch.int64, torch.int32, torch.float32]
    assert all(o.is_cuda and o.device == index.device for o in first)
    assert first[0].shape == first[1].shape == first[2].shape == (700, 5) and first[3].shape == first[4].shape == (700,)
    check([o.cpu().numpy() for o in first], S, 100.0, 5)


def test_duplicate_labels_tie_to_the_lower_label():
    index, X, _, _ = case(257, 20, 17)
    L = labels_of(17, 20).copy()
    L[9] = L[3]
    L[16] = L[3]
    S = witness(index, L)
    for t in (5, TMAX):
        D, P, J, count, Z = got = tagging.tag_rows(index, L, t)
        check(got, S, 100.0, t)
        for j in range(257):
            at = J[j, :count[j]].tolist()
            if 3 in at:
                p = at.index(3)
                if p + 2 < count[j]:
                    assert at[p:p + 3] == [3, 9, 16] and D[j, p] == D[j, p + 1] == D[j, p + 2] and P[j, p] == P[j, p + 2]
        if t == TMAX:
            assert (np.sort(J[:, :17], axis=1) == np.arange(17)).all()                    # every label once


def test_a_nan_label_is_no_candidate():
    index, X, _, _ = case(257, 20, 17)
    L = labels_of(17, 20).copy()
    L[5] = np.nan
    S = witness(index, L)
    assert np.isnan(S[:, 5]).all() and not np.isnan(np.delete(S, 5, 1)).any()
    D, P, J, count, Z = got = tagging.tag_rows(index, L, TMAX)
    check(got, S, 100.0, TMAX)
    assert (count == 16).all() and not (J == 5).any() and not np.isnan(P).any() and not np.isnan(Z).any()
    # nothing but NaN labels: no candidate, Z = 0
    D, P, J, count, Z = tagging.tag_rows(index, np.full((3, 20), np.nan, np.float32), 2)
    assert (count == 0).all() and (Z == 0).all() and (J == -1).all() and (P == 0).all() and (D == LOWEST).all()


def snapped_min_prob(P, bound, lo=0.02, hi=0.5):
    """(min_prob, margin): the middle of the widest gap between the observed probabilities in [lo, hi], relative margin to the nearest
    one: no P lies within `margin` (relative) of it, and margin must exceed the bound for the cut to be the definition's."""
    v = np.unique(np.concatenate([[lo, hi], P[(P > lo) & (P < hi)].astype(np.float64)]))
    i = int(np.argmax(np.diff(np.log(v))))
    mid = float(np.float32(np.sqrt(v[i] * v[i + 1])))
    return mid, min(mid / v[i], v[i + 1] / mid) - 1.0


@pytest.mark.parametrize("d,C", [(20, 17), (512, 130)])
def test_min_prob_truncates_the_list(d, C):
    index, X, L, S = case(700, d, C)
    t = 5
    D0, P0, J0, c0, Z0 = tagging.tag_rows(index, L, t)
    bound = tagging.tag_prob_bound(C, 100.0, SPREAD)
    cut, margin = snapped_min_prob(P0, bound)
    print(f"d={d} C={C}: min_prob {cut:.6f}, no P within {margin:.3e} (relative) of it, bound {bound:.3e}")
    assert margin > 2 * bound
    D, P, J, count, Z = got = tagging.tag_rows(index, L, t, min_prob=cut)
    check(got, S, 100.0, t, cut)                                                          # the definition's cut: no P is in doubt
    want = np.array([int(np.argmax(np.append(P0[j] < np.float32(cut), True))) for j in range(700)], np.int32)
    assert np.array_equal(count, want) and 0 < (count < t).sum() and (count > 0).sum() > 0
    for j in range(700):
        k = count[j]
        assert np.array_equal(bits(P[j, :k]), bits(P0[j, :k])) and np.array_equal(J[j, :k], J0[j, :k])
        assert (J[j, k:] == -1).all() and (P[j, k:] == 0).all() and (D[j, k:] == LOWEST).all()
    assert np.array_equal(bits(Z), bits(Z0))                                             # Z is that of all candidates
    assert (tagging.tag_rows(index, L, t, min_prob=2.0)[3] == 0).all()


def test_a_row_range_leaves_the_other_rows_untouched():
    index, X, L, S = case(257, 20, 17)
    full = tagging.tag_rows(index, L, 5)
    part = tagging.tag_rows(index, L, 5, row0=17, row1=65)                                # cuts a tile (17) and a block (65)
    fresh = tagging.tag_rows_ref(S[:0], 100.0, 5)
    for g, f, name in zip(part, full, NAMES):
        assert np.array_equal(bits(g[17:65]), bits(f[17:65])), name
    out_rows = np.r_[0:17, 65:257]
    assert (part[0][out_rows] == LOWEST).all() and (part[1][out_rows] == 0).all() and (part[2][out_rows] == -1).all()
    assert (part[3][out_rows] == 0).all() and (part[4][out_rows] == 0).all() and fresh[0].shape == (0, 5)
    # into the tensors of an earlier call: the lines outside the range keep what they held
    dev = index.device
    out = (torch.full((257, 5), 7.0, device=dev), torch.full((257, 5), 7.0, device=dev), torch.full((257, 5), 7, dtype=torch.int64, device=dev),
           torch.full((257,), 7, dtype=torch.int32, device=dev), torch.full((257,), 7.0, device=dev))
    got = [o.cpu().numpy() for o in tagging.tag_rows_device(index, L, 5, row0=17, row1=65, out=out)]
    for g, f, name in zip(got, full, NAMES):
        assert np.array_equal(bits(g[17:65]), bits(f[17:65])) and (g[out_rows] == 7).all(), name
    for r0, r1 in ((0, 16), (64, 257), (256, 257), (100, 100), (300, 400), (250, 1000)):
        got = tagging.tag_rows(index, L, 5, row0=r0, row1=r1)
        for g, f, name in zip(got, full, NAMES):
            assert np.array_equal(bits(g[r0:r1]), bits(f[r0:r1])), (name, r0, r1)
        assert (got[3][:r0] == 0).all() and (got[3][r1:] == 0).all()
    with pytest.raises(ValueError, match="no range"):
        tagging.tag_rows(index, L, 5, row0=5, row1=4)


def test_id_mapped_index_gives_the_rows_of_a_plain_one():
    index, X, L, S = case(257, 20, 17)
    mapped = build(X, np.random.default_rng(3).permutation(257).astype(np.int64) + 1000)
    same(tagging.tag_rows(mapped, L, 5), tagging.tag_rows(index, L, 5))
    for rank in ("mass", "votes"):
        same(tagging.tag_segments(mapped, L, SEGMENTS, 4, rank), tagging.tag_segments(index, L, SEGMENTS, 4, rank), rank, "LMVRm")


def test_scale_one_and_a_label_that_is_a_stored_row():
    index, X, L, S = case(257, 20, 17)
    r1 = check(tagging.tag_rows(index, L, 5, scale=1.0), S, 1.0, 5, what="scale=1")
    L2 = L.copy()
    L2[4] = X[100]                                                                        # P -> 1 for row 100
    S2 = witness(index, L2)
    D, P, J, count, Z = got = tagging.tag_rows(index, L2, 5, scale=100.0)
    r100 = check(got, S2, 100.0, 5, what="scale=100")
    assert J[100, 0] == 4 and P[100, 0] > 0.999 and abs(float(Z[100]) - 1.0) < 1e-3
    print(f"largest |error| / bound: scale=1 {r1:.4f}, scale=100 with a stored row as a label {r100:.4f}")
    # normalize=True: raw labels of any norm are normalised on the way in, as add(normalize=True)
    raw = (L.astype(np.float64) * np.random.default_rng(12).uniform(0.5, 3.0, (17, 1))).astype(np.float32)
    check(tagging.tag_rows(index, raw, 5, normalize=True), witness(index, raw, normalize=True), 100.0, 5, what="normalize")


def segment_inputs():
    X = drifting_chains(100, 20, seed=2, lengths=(6, 25))
    return build(X), X


@pytest.mark.parametrize("rank", ["mass", "votes"])
@pytest.mark.parametrize("C,g", [(17, 4), (5, 8), (130, TMAX)])
def test_tag_segments_equal_the_definition_on_the_kernels_own_lists(C, g, rank):
    index, X = segment_inputs()
    L = labels_of(C, 20)
    t, cut = 3, 0.05
    D, P, J, count, Z = tagging.tag_rows(index, L, t, min_prob=cut)
    for seg in (SEGMENTS, None, torch.from_numpy(SEGMENTS).to(index.device), np.array([0, 100], np.int64)):
        Lg, M, V, rows, mean = tagging.tag_segments(index, L, seg, g, rank, t, min_prob=cut)
        ref_seg = seg.cpu().numpy() if isinstance(seg, torch.Tensor) else seg
        want = tagging.tag_segments_ref(P, J, count, ref_seg, C, g, rank)
        same((Lg, M, V, rows), want, f"C={C} g={g} {rank}", ("L", "mass", "votes", "rows"))
        assert np.array_equal(mean, M.astype(np.float64) / (2.0 ** 24 * np.maximum(rows, 1)[:, None]))
        assert (mean <= 1.0 + 1e-6).all() and (Lg[:, min(g, C):] == -1).all()
    Lg, M, V, rows, mean = tagging.tag_segments(index, L, SEGMENTS, g, rank, t, min_prob=cut)
    assert rows.tolist() == np.diff(SEGMENTS).tolist() and (Lg[3] == -1).all() and (Lg[[0, 1, 2, 4, 5, 6, 7], 0] >= 0).all()
    assert int(V.sum(axis=1).max()) <= int(rows.max())


@pytest.mark.parametrize("C", (17, 130, 1000))
@pytest.mark.parametrize("d", (20, 512))
def test_the_first_label_is_the_float64_argmax_on_clear_rows(d, C):
    """A witness that does not go through our scores: where the best two float64 cosines of a row differ by more than twice the bound
    the flat index states for one float32 inner product, the first label is the float64 argmax.  At least 98 % of the rows qualify."""
    index, X, L, S = case(700, d, C)
    cos = X.astype(np.float64) @ L.astype(np.float64).T
    top2 = np.sort(cos, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * float(flat_score_bound(d, 1.0))
    print(f"d={d} C={C}: {int(clear.sum())} of 700 rows clear")
    assert clear.sum() >= 0.98 * 700
    J = tagging.tag_rows(index, L, 1)[2]
    assert np.array_equal(J[clear, 0], np.argmax(cos, axis=1)[clear])
    assert np.abs(S.astype(np.float64) - cos).max() <= float(flat_score_bound(d, 1.0))


def test_an_empty_index_and_bad_arguments():
    index = FlatIPIndex(20)
    L = labels_of(3, 20)
    D, P, J, count, Z = tagging.tag_rows(index, L, 5)
    assert D.shape == P.shape == J.shape == (0, 5) and count.shape == Z.shape == (0,)
    Lg, M, V, rows, mean = tagging.tag_segments(index, L, np.array([0, 0, 0]), 4)
    assert (Lg == -1).all() and Lg.shape == (2, 4) and rows.tolist() == [0, 0] and (M == 0).all() and (mean == 0).all()
    full, X = rows_case(65, 20)
    with pytest.raises(ValueError, match=r"C=4097 labels outside \[1,4096\]"):
        tagging.tag_rows(full, np.zeros((4097, 20), np.float32))
    out = [torch.zeros(65 * 2, dtype=t, device=full.device) for t in (torch.float32, torch.float32, torch.int64, torch.int32, torch.float32)]
    lab = torch.from_numpy(L).to(full.device)
    with pytest.raises(ValueError, match=r"top=65 outside \[1,64\]"):                      # the library's own checks
        full._call("ivr_index_tag_rows", lab, 3, False, 100.0, 65, 0.0, 0, 65, *out)
    with pytest.raises(ValueError, match="scale"):
        full._call("ivr_index_tag_rows", lab, 3, False, -1.0, 2, 0.0, 0, 65, *out)
    with pytest.raises(ValueError, match="table entries"):
        full._call("ivr_index_tag_segments", lab, 3, False, 100.0, 2, 0.0, lab, (1 << 25) // 3 + 1, 2, 0, *out[:4])


def test_the_largest_label_count_runs():
    """C = IVR_TAG_MAX_LABELS: the trip count is the only thing that grows."""
    C = _ffi.IVR_TAG_MAX_LABELS
    index, X = rows_case(65, 20)
    L = labels_of(C, 20)
    Lidx = FlatIPIndex(20)
    Lidx.add(L)
    rows = torch.from_numpy(X).to(index.device)
    Ds, Is = (o.cpu().numpy() for o in Lidx.search_device(rows, 5))                      # the flat search as the witness: exact scores, same order
    D, P, J, count, Z = tagging.tag_rows(index, L, 5)
    assert np.array_equal(J, Is) and np.array_equal(bits(D), bits(Ds)) and (count == 5).all()
    assert (Z >= 1).all() and np.all(np.diff(P, axis=1) <= 0)


def test_compat_tags_frames_and_videos():
    from ivr_amd.compat import FAISSRetriever, KeyframeMetadata
    rng = np.random.default_rng(21)
    names = ["beach", "city", "forest", "kitchen"]
    protos = unit32(rng.standard_normal((4, 32)))
    kind = np.repeat([0, 1, 2, 1, 3, 3], 5)                                              # six videos of five frames
    feats = unit32(protos[kind] + 0.05 * rng.standard_normal((30, 32)))
    metas = [KeyframeMetadata(folder_name=f"L01_V{i // 5:03d}", image_name=f"{i % 5:03d}.jpg", frame_id=i % 5, file_path=f"/k/{i}.jpg",
                              clip_features=feats[i]) for i in range(30)]
    metas[0].scene_tags = ["kitchen", "handmade"]
    r = FAISSRetriever()
    r.build_index(feats, metas)
    found = r.tag_frames(names, protos * 2.0, top=2, min_prob=0.1)                        # labels of any norm: normalised here
    assert len(found) == 30
    for i, m in enumerate(metas):
        assert found[m.get_unique_key()][0] == names[kind[i]]
        assert m.scene_tags[-len(found[m.get_unique_key()]):] == found[m.get_unique_key()] or i == 0
    assert metas[0].scene_tags[:2] == ["kitchen", "handmade"] and metas[0].scene_tags[2] == "beach"       # appended, order kept
    before = [list(m.scene_tags) for m in metas]
    r.tag_frames(names, protos, top=2, min_prob=0.1)
    assert [m.scene_tags for m in metas] == before                                       # a second pass adds no duplicate
    videos = r.tag_videos(names, protos, top_labels=2, rank="votes")
    assert list(videos) == [f"L01_V{v:03d}" for v in range(6)]
    assert [videos[f"L01_V{v:03d}"][0][0] for v in range(6)] == ["beach", "city", "forest", "city", "kitchen", "kitchen"]
    mass = r.tag_videos(names, protos, top_labels=4, rank="mass")
    for v in range(6):
        tags = mass[f"L01_V{v:03d}"]
        assert tags[0][0] == videos[f"L01_V{v:03d}"][0][0] and 0.5 < tags[0][1] <= 1.0
        assert [p for _, p in tags] == sorted((p for _, p in tags), reverse=True)
    with pytest.raises(ValueError, match="label_features"):
        r.tag_frames(names, protos[:3])
