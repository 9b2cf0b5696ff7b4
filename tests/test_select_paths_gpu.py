"""GPU: select_topk_kernel (csrc/search_select.h) on every path of its dispatch, fed directly through the two shard-merge entry
points (topk_merge: SrcParts / OUT_DI_PARTS, topk_merge_packed: SrcPacked / OUT_DI_PACKED) with n = parts * k keys per query.
The kernel sorts, so the comparison with the host sort oracle.search_ref.select_ref is exact: ids equal, scores equal bit for bit
(a -0.0 may come back as +0.0).  Which branch a case takes is proved on the CPU (tests/test_select_ref_cpu.py) for the same
case table (tests/select_cases.py)."""
import numpy as np
import pytest
import torch

import select_cases as T
from oracle import search_ref as S

pytestmark = pytest.mark.gpu

NEG_ZERO = np.uint32(0x80000000)


def _merge_both(D_parts, I_parts, per_part_pack=False):
    """(D, I) of topk_merge and of topk_merge_packed for the same candidates, as numpy arrays."""
    from ivr_amd.index import topk_merge, topk_merge_packed, topk_pack
    parts, nq, k = D_parts.shape
    Dp, Ip = torch.from_numpy(np.array(D_parts)).cuda(), torch.from_numpy(np.array(I_parts)).cuda()
    Da, Ia = topk_merge(Dp, Ip)
    if per_part_pack:
        packed = torch.stack([topk_pack(d, i) for d, i in zip(Dp, Ip)])
    else:                                       # the pack is per element: one call over all parts gives the same buffer
        packed = topk_pack(Dp.reshape(parts * nq, k), Ip.reshape(parts * nq, k)).reshape(parts, nq, k, 3)
    Dk, Ik = topk_merge_packed(packed)
    return Da.cpu().numpy(), Ia.cpu().numpy(), Dk.cpu().numpy(), Ik.cpu().numpy()


def _check(la, per_part_pack=False):
    D_parts, I_parts = la.arrays()
    Dr, Ir = S.select_ref(D_parts, I_parts, la.k)
    Da, Ia, Dk, Ik = _merge_both(D_parts, I_parts, per_part_pack)
    for q in range(la.nq):
        bad = np.nonzero(Ia[q] != Ir[q])[0]
        assert bad.size == 0, (la, q, la.queries[q], "first wrong slot", bad[0], Ia[q][bad[:4]], Ir[q][bad[:4]])
    got, want = Da.view(np.uint32), Dr.view(np.uint32)
    assert np.array_equal(Da, Dr), la                                               # by value (there is no NaN)
    assert ((got == want) | ((want == NEG_ZERO) & (got == 0))).all(), la            # by bits, but for -0.0 -> +0.0
    assert np.array_equal(Ik, Ia) and np.array_equal(Dk.view(np.uint32), got), la   # packed = arrays, bit for bit


@pytest.mark.parametrize("la", T.LAUNCHES, ids=repr)
def test_merge_equals_host_sort_on_every_path(la):
    _check(la, per_part_pack=la.parts <= 64)


def test_unused_slots_and_special_values():
    """Nothing valid: every slot is (-FLT_MAX, -1) whatever the absent slots carry as scores.  -FLT_MAX under a valid id keeps its id,
    -inf ranks below it, the zeros tie by position, the denormals keep their order."""
    for parts, k in ((16, 256), (410, 10), (1700, 10)):
        D_parts = np.full((parts, 2, k), T.ABSENT_SCORE, dtype=np.float32)
        Da, Ia, Dk, Ik = _merge_both(D_parts, np.full((parts, 2, k), -1, dtype=np.int64))
        for D, I in ((Da, Ia), (Dk, Ik)):
            assert (I == -1).all() and (D.view(np.uint32) == S.NEG_FLT_MAX.view(np.uint32)).all(), (parts, k)
    vals = np.array([-2e-40, -0.0, -np.inf, 2e-40, 0.0, S.NEG_FLT_MAX, 1e-40, np.inf, -1e-40, 3.0e38], dtype=np.float32)
    ids = np.array([7, 5, 0, 1 << 35, 3, 9, 2, 8, 4, -1], dtype=np.int64)             # the last one absent; a valid id 0
    Da, Ia, Dk, Ik = _merge_both(vals.reshape(1, 1, 10), ids.reshape(1, 1, 10))
    assert Ia[0].tolist() == [8, 1 << 35, 2, 5, 3, 4, 7, 9, 0, -1] and np.array_equal(Ik, Ia)
    want = np.array([np.inf, 2e-40, 1e-40, 0.0, 0.0, -1e-40, -2e-40, S.NEG_FLT_MAX, -np.inf, S.NEG_FLT_MAX], dtype=np.float32)
    assert np.array_equal(Da[0], want) and np.array_equal(Dk[0], want)
    assert (Da[0][[1, 2, 5, 6]] != 0).all()                                            # denormals are not flushed


def test_random_sweep_equals_host_sort():
    for la in T.sweep_launches():
        _check(la)


def test_api_errors():
    from ivr_amd import _ffi
    from ivr_amd.index import topk_merge, topk_merge_packed
    k = _ffi.IVR_MAX_K + 1
    D = torch.zeros((2, 1, k), dtype=torch.float32, device="cuda")
    I = torch.zeros((2, 1, k), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        topk_merge(D, I)                                                  # k > IVR_MAX_K
    with pytest.raises(ValueError):
        topk_merge_packed(torch.zeros((2, 1, k, 3), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        topk_merge(D[:, :, :10].contiguous(), I[:, :, :10].contiguous(), k=5)     # k differs from the per-part k
