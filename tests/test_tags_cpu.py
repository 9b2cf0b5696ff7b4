"""CPU suite of the zero-shot tagging (ivr_amd/tagging.py, csrc/tags.hip): the two numpy definitions against a literal float64
restatement (torch.softmax on the CPU, argsort), ties, a NaN label, the min_prob truncation, the segment conventions, the fixed-point
mass, the derived bound, the ABI of the four new entry points and the argument checks that need no device.  No compute call reaches
a device."""
import ctypes
import re

import numpy as np
import pytest
import torch

from cluster_cases import SEGMENTS, drifting_chains, unit32
from conftest import ROOT
from ivr_amd import _ffi, _staging, tagging
from ivr_amd.index import FlatIPIndex

NEW = ("ivr_tag_max_labels", "ivr_tag_max_top", "ivr_index_tag_rows", "ivr_index_tag_segments")
LOWEST = np.float32(-np.finfo(np.float32).max)


def labels_of(C, d):
    return unit32(np.random.default_rng([7, C, d]).standard_normal((C, d)))


def scores32(X, L):
    return (X @ L.T).astype(np.float32)


# -- the definitions against a literal restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("N,d,C,t", [(257, 20, 17, 5), (64, 512, 130, 64), (65, 20, 1, 1), (16, 20, 3, 5)])
def test_tag_rows_ref_is_the_float64_softmax_and_argsort(N, d, C, t, scale):
    S = scores32(drifting_chains(N, d), labels_of(C, d))
    D, P, J, count, Z = tagging.tag_rows_ref(S, scale, t)
    assert (D.dtype, P.dtype, J.dtype, count.dtype, Z.dtype) == (np.float32, np.float32, np.int64, np.int32, np.float32)
    assert D.shape == P.shape == J.shape == (N, t) and count.shape == Z.shape == (N,)
    soft = torch.softmax(torch.from_numpy(S.astype(np.float64)) * float(np.float32(scale)), dim=1).numpy()
    order = np.argsort(-S.astype(np.float64), axis=1, kind="stable")[:, :t]            # stable: equal scores the lower label
    u = min(t, C)
    assert (count == u).all()
    assert np.array_equal(J[:, :u], order) and (J[:, u:] == -1).all() and (D[:, u:] == LOWEST).all() and (P[:, u:] == 0).all()
    assert np.array_equal(D[:, :u], np.take_along_axis(S, order, 1))
    want = np.take_along_axis(soft, order, 1)
    assert np.abs(P[:, :u] - want).max() <= 2.0 ** -24 * want.max() + 1e-45           # the float64 value rounded once
    m = S.astype(np.float64).max(axis=1, keepdims=True)
    Z64 = np.exp(float(np.float32(scale)) * (S.astype(np.float64) - m)).sum(axis=1)
    assert np.allclose(Z, Z64, rtol=2.0 ** -23, atol=0) and (Z >= 1).all()
    if u > 1:
        assert (np.diff(P[:, :u].astype(np.float64), axis=1) <= 0).all()                # P descends with the rank


def test_ties_nan_labels_negative_zero_and_the_truncation():
    S = np.array([[0.5, 0.9, 0.9, 0.1],                    # a tie: the lower label first
                  [np.nan, 0.2, np.nan, 0.3],              # NaN labels: no candidates, not in Z
                  [np.nan, np.nan, np.nan, np.nan],        # no candidate at all
                  [-0.0, 0.0, -0.5, -0.5]], np.float32)    # -0.0 counts as +0.0 and ties with it
    D, P, J, count, Z = tagging.tag_rows_ref(S, 10.0, 3)
    assert J.tolist() == [[1, 2, 0], [3, 1, -1], [-1, -1, -1], [0, 1, 2]] and count.tolist() == [3, 2, 0, 3]
    assert D[3, 0].view(np.uint32) == 0 and D[3, 1].view(np.uint32) == 0
    assert P[0, 0] == P[0, 1] and Z[2] == 0 and (P[2] == 0).all() and (D[2] == LOWEST).all()
    z1 = 1.0 + np.exp(10.0 * (np.float64(np.float32(0.2)) - np.float64(np.float32(0.3))))
    assert Z[1] == np.float32(z1) and P[1, 0] == np.float32(1.0 / z1) and P[1, 1] == np.float32((z1 - 1.0) / z1)
    assert abs(float(P[1, :2].sum()) - 1.0) < 1e-6
    # min_prob cuts the list at the first slot below float32(min_prob); Z is that of all candidates
    p = P[0]
    for cut, want in ((0.0, 3), (float(p[2]), 3), (float(np.nextafter(p[2], np.float32(1))), 2), (float(p[0]), 2),
                      (float(np.nextafter(p[0], np.float32(1))), 0), (2.0, 0), (-1.0, 3)):
        Dc, Pc, Jc, cc, Zc = tagging.tag_rows_ref(S, 10.0, 3, cut)
        assert cc[0] == want and Zc[0] == Z[0], cut
        assert np.array_equal(Pc[0, :want], P[0, :want]) and (Pc[0, want:] == 0).all() and (Jc[0, want:] == -1).all()
        assert (Dc[0, want:] == LOWEST).all()
    assert tagging.tag_rows_ref(S, 10.0, 4)[3].tolist() == [4, 2, 0, 4]


def rows_for_segments(t=3, C=6):
    rng = np.random.default_rng(5)
    S = rng.uniform(-1, 1, (100, C)).astype(np.float32)
    return tagging.tag_rows_ref(S, 4.0, t, 0.05)


@pytest.mark.parametrize("rank", ["mass", "votes"])
def test_tag_segments_ref_follows_the_segment_conventions(rank):
    D, P, J, count, Z = rows_for_segments()
    C, g = 6, 4
    L, M, V, rows = tagging.tag_segments_ref(P, J, count, SEGMENTS, C, g, rank)
    nseg = len(SEGMENTS) - 1
    assert L.shape == M.shape == V.shape == (nseg, g) and rows.shape == (nseg,)
    assert (L.dtype, M.dtype, V.dtype, rows.dtype) == (np.int64, np.uint64, np.int32, np.int32)
    assert rows.tolist() == np.diff(SEGMENTS).tolist()                          # row 0 and rows 90 .. 99 are counted nowhere
    for s in range(nseg):
        lo, hi = int(SEGMENTS[s]), int(SEGMENTS[s + 1])
        mass, votes = {}, {}
        for j in range(lo, hi):                                                # the literal restatement
            for p in range(count[j]):
                fixed = int(np.rint(np.float64(P[j, p]) * 2.0 ** 24))
                mass[int(J[j, p])] = mass.get(int(J[j, p]), 0) + fixed
            if count[j]:
                votes[int(J[j, 0])] = votes.get(int(J[j, 0]), 0) + 1
        value = mass if rank == "mass" else votes
        want = sorted(value, key=lambda i: (-value[i], i))[:g]
        assert L[s, :len(want)].tolist() == want and (L[s, len(want):] == -1).all()
        assert M[s, :len(want)].tolist() == [mass.get(i, 0) for i in want] and (M[s, len(want):] == 0).all()
        assert V[s, :len(want)].tolist() == [votes.get(i, 0) for i in want] and (V[s, len(want):] == 0).all()
    assert (L[3] == -1).all() and rows[3] == 0                                  # the empty segment [17, 17)
    # one segment over everything is the call without segments; g beyond C leaves unused slots
    a = tagging.tag_segments_ref(P, J, count, None, C, 8, rank)
    b = tagging.tag_segments_ref(P, J, count, np.array([0, 100]), C, 8, rank)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[3].tolist() == [100] and (a[0][0, C:] == -1).all()


def test_the_mass_is_an_exact_fixed_point_sum():
    P = np.array([[0.75, 0.25], [2.0 ** -24, 2.0 ** -25], [1.0, 0.0], [0.6, 0.4]], np.float32)
    J = np.array([[1, 0], [1, 0], [0, -1], [0, 1]], np.int64)
    count = np.array([2, 2, 1, 2], np.int32)
    L, M, V, rows = tagging.tag_segments_ref(P, J, count, None, 2, 2, "mass")
    f = lambda x: int(np.rint(np.float64(np.float32(x)) * 2.0 ** 24))          # noqa: E731
    # 2^-25 2^24 = 0.5 rounds to even: 0
    want = {0: f(0.25) + 0 + f(1.0) + f(0.6), 1: f(0.75) + 1 + f(0.4)}
    assert L.tolist() == [[0, 1]] and M.tolist() == [[want[0], want[1]]] and V.tolist() == [[2, 2]] and rows.tolist() == [4]
    assert tagging.tag_segments_ref(P, J, count, None, 2, 2, "votes")[0].tolist() == [[0, 1]]      # a tie in votes: the lower label
    assert tagging.MASS_ONE == 1 << 24


def test_the_bound_is_the_derivation():
    u = 2.0 ** -24
    b = tagging.tag_prob_bound(1000, 100.0, 2.0)
    T = 8                                                                       # ceil(ceil(1000 / 16) / 8)
    assert b == pytest.approx(1.01 * (2 * (2 * u * 100 * 2) + u * (3 * (T + 1) + 2 + 4 * T + 32 + 3)), rel=1e-12)
    assert 4.7e-5 < b < 1e-4
    assert tagging.tag_prob_bound(1, 1.0, 2.0) < 5e-6
    assert tagging.tag_prob_bound(4096, 100.0, 2.0) > b > tagging.tag_prob_bound(1000, 100.0, 1.0)


# -- ABI and surfaces ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/ivr_api.h").read(), flags=re.S)


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl or decl.startswith("ivr_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


@pytest.mark.parametrize("name,names", [
    (NEW[0], []), (NEW[1], []),
    (NEW[2], ["idx", "labels", "C", "normalize", "scale", "t", "min_prob", "row0", "row1", "D", "P", "J", "count", "Z", "stream"]),
    (NEW[3], ["idx", "labels", "C", "normalize", "scale", "t", "min_prob", "seg_off", "nseg", "g", "rank", "L", "mass", "votes", "rows",
              "stream"])])
def test_header_binding_and_library_agree(name, names):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} not declared in ivr_api.h"
    params = [p.strip() for p in m.group(1).split(",") if p.strip() != "void"]
    assert [re.sub(r"[\s*]+", " ", p).split()[-1] for p in params] == names
    res, args = _ffi._SIGS[name]
    assert res is ctypes.c_int and args == [_ctype_of(p) for p in params]
    if names:
        assert _ffi._STREAM[name] == len(params) - 1 and name not in _ffi._VALUE
    else:
        assert name not in _ffi._STREAM and name in _ffi._VALUE
    assert name in _ffi.EXPORTS
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)


def test_limits_of_the_library():
    assert re.search(r"#define\s+IVR_TAG_MAX_LABELS\s+4096\b", _header()) and re.search(r"#define\s+IVR_TAG_MAX_TOP\s+64\b", _header())
    assert tagging.tag_max_labels() == _ffi.IVR_TAG_MAX_LABELS == 4096
    assert tagging.tag_max_top() == _ffi.IVR_TAG_MAX_TOP == 64
    assert _ffi.IVR_TAG_RANK == {"mass": 0, "votes": 1}
    assert re.search(r"#define\s+IVR_TAG_RANK_MASS\s+0\b", _header()) and re.search(r"#define\s+IVR_TAG_RANK_VOTES\s+1\b", _header())
    assert _ffi.API_VERSION == 11 and _ffi.load().ivr_api_version() == 11        # additions only


def test_library_rejects_bad_arguments_before_any_device_call():
    lib = _ffi.load()
    err = lambda: lib.ivr_last_error(None)                                      # noqa: E731
    assert lib.ivr_index_tag_rows(None, None, 1, 0, 100.0, 1, 0.0, 0, 0, None, None, None, None, None, None) == -1
    assert b"NULL" in err()
    assert lib.ivr_index_tag_segments(None, None, 1, 0, 100.0, 1, 0.0, None, 0, 1, 0, None, None, None, None, None) == -1
    assert b"NULL" in err()
    fake = ctypes.create_string_buffer(64)                 # stands for the handle and the outputs: a rejected call reads none of them
    p = ctypes.cast(fake, ctypes.c_void_p)
    rows = lambda C=4, scale=100.0, t=2, mp=0.0, r0=0, r1=0, lab=p: lib.ivr_index_tag_rows(          # noqa: E731
        p, lab, C, 0, scale, t, mp, r0, r1, p, p, p, p, p, None)
    segs = lambda C=4, scale=100.0, t=2, mp=0.0, seg=None, nseg=0, g=2, rank=0: lib.ivr_index_tag_segments(          # noqa: E731
        p, p, C, 0, scale, t, mp, seg, nseg, g, rank, p, p, p, p, None)
    assert rows(lab=None) == -1 and b"NULL labels" in err()
    for C in (0, -1, 4097):
        assert rows(C=C) == -1 and f"C={C} outside [1,4096]".encode() in err()
        assert segs(C=C) == -1 and f"C={C} outside [1,4096]".encode() in err()
    for t in (0, 65):
        assert rows(t=t) == -1 and f"top={t} outside [1,64]".encode() in err()
        assert segs(t=t) == -1 and f"top={t} outside [1,64]".encode() in err()
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert rows(scale=scale) == -1 and b"scale=" in err()
        assert segs(scale=scale) == -1 and b"scale=" in err()
    assert rows(mp=float("nan")) == -1 and b"min_prob" in err()
    assert segs(mp=float("nan")) == -1 and b"min_prob" in err()
    assert rows(r0=5, r1=4) == -1 and b"[5,4) are no range" in err()
    assert rows(r0=-1, r1=4) == -1 and b"no range" in err()
    for g in (0, 65):
        assert segs(g=g) == -1 and f"top_labels={g} outside [1,64]".encode() in err()
    assert segs(rank=2) == -1 and b"rank=2" in err()
    assert segs(seg=p, nseg=0) == -1 and b"nseg=0" in err()
    assert segs(C=4096, seg=p, nseg=(1 << 25) // 4096 + 1) == -1 and b"table entries" in err()


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("tag_rows", "tag_rows_device", "tag_segments", "tag_segments_device", "tag_rows_ref", "tag_segments_ref",
                 "tag_prob_bound", "zero_shot_labels"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(tagging, name)


def test_argument_checks_name_the_offending_values():
    index = FlatIPIndex.__new__(FlatIPIndex)             # no handle: every check below fails before the library is called
    index.d, index.device = 8, torch.device("cpu")
    lab = np.zeros((3, 8), np.float32)
    with pytest.raises(ValueError, match="FlatIPIndex"):
        tagging.tag_rows_device(object(), lab)
    with pytest.raises(ValueError, match=r"labels expects \[n,8\], got \(3, 5\)"):
        tagging.tag_rows_device(index, np.zeros((3, 5), np.float32))
    with pytest.raises(ValueError, match=r"labels expects \[n,8\]"):
        tagging.tag_segments_device(index, np.zeros(8, np.float32))
    for fn in (tagging.tag_rows_device, tagging.tag_segments_device):
        with pytest.raises(ValueError, match=r"C=0 labels outside \[1,4096\]"):
            fn(index, np.zeros((0, 8), np.float32))
        with pytest.raises(ValueError, match=r"top=0 outside \[1,64\]"):
            fn(index, lab, top=0)
        with pytest.raises(ValueError, match=r"top=65 outside \[1,64\]"):
            fn(index, lab, top=65)
        with pytest.raises(ValueError, match="top must be an integer, got float"):
            fn(index, lab, top=2.0)
        with pytest.raises(ValueError, match="scale=0.0 is not a positive finite number"):
            fn(index, lab, scale=0)
        with pytest.raises(ValueError, match="scale=nan is not a positive finite number"):
            fn(index, lab, scale=float("nan"))
        with pytest.raises(ValueError, match="scale must be a number, got str"):
            fn(index, lab, scale="100")
        with pytest.raises(ValueError, match="min_prob=nan is NaN"):
            fn(index, lab, min_prob=float("nan"))
    with pytest.raises(ValueError, match=r"top_labels=65 outside \[1,64\]"):
        tagging.tag_segments_device(index, lab, top_labels=65)
    with pytest.raises(ValueError, match="rank must be 'mass' or 'votes', got 'mean'"):
        tagging.tag_segments_device(index, lab, rank="mean")
    with pytest.raises(ValueError, match=r"seg_off\[1\]=5 > seg_off\[2\]=3"):
        tagging.tag_segments_device(index, lab, seg_off=np.array([0, 5, 3]))
    assert _staging.check_row_range(0, None, 7, "x") == (0, 7) and _staging.check_row_range(17, 65, 40, "x") == (17, 40)
    assert _staging.check_row_range(9, 12, 4, "x") == (9, 9)
    with pytest.raises(ValueError, match=r"rows \[5,4\) are no range"):
        _staging.check_row_range(5, 4, 10, "tag_rows")
    with pytest.raises(ValueError, match=r"rows \[-1,4\) are no range"):
        _staging.check_row_range(-1, 4, 10, "tag_rows")
    with pytest.raises(ValueError, match="row0 must be an integer, got float"):
        _staging.check_row_range(1.0, 4, 10, "tag_rows")
    with pytest.raises(ValueError, match=r"top=65 outside"):
        tagging.tag_rows_ref(np.zeros((2, 2), np.float32), 1.0, 65)
    with pytest.raises(ValueError, match=r"must be \[n,C\]"):
        tagging.tag_rows_ref(np.zeros(3, np.float32))


def test_zero_shot_labels_go_through_encode_text():
    class Extractor:
        def encode_text(self, texts):
            self.texts = list(texts)
            return np.arange(len(texts) * 4, dtype=np.float64).reshape(len(texts), 4)
    e = Extractor()
    out = tagging.zero_shot_labels(e, ["cat", "dog"])
    assert e.texts == ["a photo of a cat", "a photo of a dog"] and out.dtype == np.float32 and out.shape == (2, 4)
    tagging.zero_shot_labels(e, ["cat"], template="{} on video")
    assert e.texts == ["cat on video"]
    with pytest.raises(ValueError, match="non-empty strings"):
        tagging.zero_shot_labels(e, ["cat", " "])
    with pytest.raises(ValueError, match="non-empty strings"):
        tagging.zero_shot_labels(e, [])
