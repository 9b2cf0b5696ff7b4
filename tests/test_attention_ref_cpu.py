"""CPU suite: the float64 attention reference and its per-element bound (oracle/attention_ref.py) are neither too loose nor too
tight.  A numpy emulation of a correct flash kernel (float32 scores, 32-key blocks with a running max, P rounded to bf16 before the
PV product, float32 row sums, bf16 / e4m3 / float32 output) passes every check the GPU tests make, with margin; the same emulation
with a typical kernel fault fails at least one of them - at T = 257 and 577 too, where the pooled-embedding checks of the tower
tests cannot see such a fault."""
import numpy as np
import pytest
import torch

from oracle import attention_ref as A

FAULTS = ("drop_last", "pad_leak", "rot_last_tile", "rot_rows_16_31", "diag_plus", "diag_minus", "skip_rescale", "cross_image",
          "v_transpose")


def emulate(q, k, v, causal, out_kind, fault=None):
    """Flash attention as the kernels compute it, on [n, H, T, 64] float32 operands -> float64 output values [n, H, T, 64]."""
    n, H, T, _ = q.shape
    Tp = -(-T // 32) * 32
    out = np.empty((n, H, T, 64), np.float64)
    rows = np.arange(T)
    for a in range(n):
        for h in range(H):
            qq = q[a, h]
            kk = k[(a + 1) % n, h] if fault == "cross_image" else k[a, h]
            vv = v[a, h].copy()
            if fault == "v_transpose":
                for j0 in range(0, T - 15, 16):
                    for d0 in range(0, 64, 16):
                        vv[j0:j0 + 16, d0:d0 + 16] = vv[j0:j0 + 16, d0:d0 + 16].T.copy()
            nkeys = Tp if fault == "pad_leak" else T
            kx = np.zeros((nkeys, 64), np.float32)
            vx = np.zeros((nkeys, 64), np.float32)
            kx[:T], vx[:T] = kk, vv
            # per-row V as the row reads it (row / key slips)
            shift = np.zeros(T, np.int64)
            if fault == "rot_last_tile":
                shift[16 * ((T - 1) // 16):] = 1
            if fault == "rot_rows_16_31":
                shift[16:32] = 3
            m = np.full(T, -np.inf, np.float32)
            l = np.zeros(T, np.float32)
            o = np.zeros((T, 64), np.float32)
            for b, k0 in enumerate(range(0, nkeys, 32)):
                keys = np.arange(k0, min(k0 + 32, nkeys))
                s = (qq @ kx[keys].T).astype(np.float32)                    # float32 accumulation
                allowed = np.ones_like(s, dtype=bool)
                if fault == "drop_last":
                    allowed &= keys[None, :] != T - 1
                if causal:
                    lim = rows + (1 if fault == "diag_plus" else -1 if fault == "diag_minus" else 0)
                    lim = np.maximum(lim, 0)
                    allowed &= keys[None, :] <= lim[:, None]
                s = np.where(allowed, s, np.float32(-np.inf))
                mn = np.maximum(m, s.max(axis=1))
                if not (fault == "skip_rescale" and b == 1):
                    alpha = np.where(m == -np.inf, np.float32(0), np.exp(m - mn)).astype(np.float32)
                    l *= alpha
                    o *= alpha[:, None]
                m = mn
                p = np.where(np.isfinite(s), np.exp(s - m[:, None]), 0).astype(np.float32)
                l += p.sum(axis=1, dtype=np.float32)
                if out_kind != "f32":
                    p = torch.from_numpy(p).to(torch.bfloat16).to(torch.float32).numpy()
                vk = vx[np.where(keys[None, :] < T, (keys[None, :] + shift[:, None]) % T, keys[None, :])] if shift.any() else vx[keys]
                if shift.any():
                    o += np.einsum("ij,ijd->id", p, vk).astype(np.float32)
                else:
                    o += (p @ vk).astype(np.float32)
            out[a, h] = A.round_to((o * (np.float32(1) / l)[:, None]).astype(np.float64), out_kind)
    return out


def fault_applies(fault, T, causal, n):
    if fault in ("diag_plus", "diag_minus"):
        return causal and T > 1
    if fault == "pad_leak":                   # under the causal mask the padded keys lie past every row's diagonal
        return T % 32 != 0 and not causal
    if fault == "skip_rescale":
        return T > 32
    if fault == "rot_rows_16_31":
        return T > 16
    if fault == "cross_image":
        return n > 1
    if fault == "v_transpose":
        return T >= 16
    return T > 1


def shape_cases():
    # (n, H, T): every kernel class of the GPU test - short (T <= 64), head-resident (65..640), generic (> 640)
    return [(3, 1, 1), (3, 1, 17), (2, 2, 64), (3, 1, 65), (2, 2, 257), (2, 1, 577), (1, 1, 1024)]


def run_checks(n, H, T, causal, out_kind, fault=None, seed=0):
    """Every check of the GPU test on the emulation -> {design: max violation ratio}; > 1 fails."""
    rng = np.random.default_rng(seed + T + 7 * causal)
    res = {}
    q, k, v = A.design_uniform(rng, n, H, T)
    got = emulate(q, k, v, causal, out_kind, fault)
    ok = A.within_ulps(got, A.uniform_expected(v, causal), out_kind, 2 if out_kind == "f32" else 1)
    res["uniform"] = 0.0 if ok.all() else np.inf
    q, k, v, pis = A.design_onehot(rng, n, H, T, causal)
    got = emulate(q, k, v, causal, out_kind, fault)
    res["onehot"] = 0.0 if np.array_equal(got, A.onehot_expected(v, pis)) else np.inf
    for name, std, off in (("gauss0.3", 0.3, 0), ("gauss3", 3.0, 0), ("gauss10", 10.0, 0), ("near1e3", 3.0, 1000.0)):
        q, k, v = A.design_gaussian(rng, n, H, T, std, off)
        got = emulate(q, k, v, causal, out_kind, fault)
        qkv = torch.from_numpy(A.pack(q, k, v))
        ref, absv, eps = A.attention_ref(qkv, T, H, causal)
        err = np.abs(got - A.unpack(ref.numpy(), n, T, H))
        bound = A.unpack(A.attention_bound(ref, absv, eps, out_kind, T).numpy(), n, T, H)
        res[name] = float((err / bound).max())
    return res


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("n,H,T,out_kind", [c + (o,) for c in shape_cases() for o in ("bf16", "e4m3", "f32")
                                             if o != "f32" or c[2] <= 512])
def test_correct_kernel_passes_with_margin(n, H, T, causal, out_kind):
    res = run_checks(n, H, T, causal, out_kind)
    print(f"T={T} causal={causal} {out_kind}: " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
    assert res["uniform"] == 0 and res["onehot"] == 0, res
    for k in ("gauss0.3", "gauss3", "gauss10", "near1e3"):
        assert res[k] <= 0.95, (k, res)       # the rounding terms are attained by design (see the oracle's docstring)


@pytest.mark.parametrize("out_kind", ["bf16", "e4m3"])
@pytest.mark.parametrize("fault,T,causal", [(f, T, c) for f in FAULTS for T in (65, 257, 577) for c in (False, True)
                                            if fault_applies(f, T, c, 2)])
def test_every_fault_is_rejected(fault, T, causal, out_kind):
    n, H = 2, 1
    res = run_checks(n, H, T, causal, out_kind, fault=fault)
    caught = [k for k, v in res.items() if v > 1]
    print(f"{fault} T={T} causal={causal} {out_kind}: rejected by {caught}  " + " ".join(f"{k}={v:.3g}" for k, v in res.items()))
    assert caught, f"fault {fault} passes every check: {res}"


def test_onehot_codes_separate():
    rng = np.random.default_rng(3)
    for T in (1, 64, 641, 1024):
        c = A.onehot_codes(rng, T)
        g = c @ c.T
        np.fill_diagonal(g, -64)
        assert g.max() <= 40 and (c @ c.T).diagonal().min() == 64
        pi = A.onehot_targets(T, True, rng, edges=(96, 192))
        assert (pi <= np.arange(T)).all() and pi[T - 1] == T - 1


def test_bound_is_tight_enough():
    # the dropped last key moves one row by a_last |v_last - out|: with one dominant key (the last) that is O(1), far outside
    q = np.zeros((1, 1, 40, 64), np.float32)
    k = np.zeros_like(q)
    v = np.ones_like(q)
    q[0, 0, :, 0] = 1.0
    k[0, 0, -1, 0] = 8.0
    v[0, 0, -1] = -1.0
    ref, absv, eps = A.attention_ref(torch.from_numpy(A.pack(q, k, v)), 40, 1, False)
    bound = A.attention_bound(ref, absv, eps, "bf16", 40)
    assert float(bound.max()) < 0.02
    got = emulate(q, k, v, False, "bf16", "drop_last")
    assert np.abs(got - A.unpack(ref.numpy(), 1, 40, 1)).max() > 0.5
