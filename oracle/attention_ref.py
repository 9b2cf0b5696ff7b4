"""ORACLE (test infrastructure, never shipped, never imported by the product path).

float64 restatement of the two tower kernels that are not GEMMs, for the per-element tests of ivr_attention /
ivr_qkv_attention / ivr_layernorm (tests/test_attention_gpu.py, tests/test_layernorm_gpu.py): softmax(Q K^T [+ causal mask]) V per
(image, head) as in modeling_clip.py:259-277 (the 1/sqrt(64) scale is folded into the Q weights by the towers, so none here), and
nn.LayerNorm.  The operands are taken exactly as the kernels read them (bf16 / e4m3 / float32 decoded to float64), so the only
difference between kernel and reference is the kernel's own rounding, which `attention_bound` / `layernorm_bound` bound per
element.  Everything is torch, so the large references run on the GPU in float64.

Error bound of the attention kernels (u = 2^-24, one query row i, weights a_j = softmax_j, V column d):

  * scores.  s_ij = q_i . k_j accumulates 64 products in float32 (MFMA or FMA chain): |ds_ij| <= 64 u sum_d |q_id||k_jd|.  The
    exponent argument (s_ij - m_i) * log2(e) is rounded once more: relative error of p_ij <= 2u |s_ij - m_i|.  With
        eps_i = 64 u max_j sum_d |q_id||k_jd| + 2u max_j |s_ij - m_i| + 2u      (the last term: v_exp_f32 is exact to 1 ulp)
    every p_ij is off by a factor in [e^-eps, e^eps] relative to the others, so each a_j moves by at most 2 eps_i a_j (numerator and
    denominator) and the output by at most 2 eps_i sum_j a_j |v_jd| = 2 eps_i (a @ |v|)_id.
  * bf16 kernels: P is rounded to bf16 (round to nearest even, unit roundoff 2^-8: 8 significant bits) before the PV product,
    the row sum l uses the unrounded float32 p: <= 2^-8 (a @ |v|).  The PV accumulation in float32 over T <= 1024 keys adds
    <= T u (a @ |v|) <= 2^-14 (a @ |v|) (2^-13 covers it with the cross terms); the final 1/l (v_rcp_f32, 1 ulp) and the product
    o / l add 4 u |ref|.  Before the output rounding:
        pre = (2^-8 + 2^-13 + 2 eps) (a @ |v|) + 4 u |ref|
    The output rounding adds 2^-8 |out| for bf16 and 2^-4 |out| for e4m3 (3 mantissa bits; plus 2^-10 absolute below the
    smallest normal 2^-6, where the spacing is 2^-9), and |out| <= |ref| + pre:
        bf16:  |out - ref| <= (1 + 2^-8) pre + 2^-8 |ref|
        e4m3:  |out - ref| <= (1 + 2^-4) pre + 2^-4 |ref| + 2^-10
    Every term is a worst case that random operands approach (P and output roundings of half an ulp), so a correct kernel reaches
    ~0.7 (bf16) to ~0.9 (e4m3) of the bound on Gaussian inputs; no term has slack to spare for a missing or extra key.
  * float32 kernel (no P rounding): the PV sum and the online rescales (one multiply per key at most) are serial float32 chains of
    at most T links, the KS-lane merge adds log2(8) more, the division 2 ulp:
        f32:   |out - ref| <= ((2 T + 16) u + 2 eps) (a @ |v|) + 4 u |ref|

tests/test_attention_ref_cpu.py checks on the CPU that a numpy emulation of a correct flash kernel stays inside these bounds with margin
and that the typical kernel faults (dropped / leaked keys, mask off by one, skipped rescale, row / key / image slips) leave them.

LayerNorm (layernorm_kernel: one wave per row, two-pass statistics in float32 on d = x - x0, x0 = the row's first element; the
subtraction is exact wherever x and x0 are within a factor 2, in particular for constant rows, which therefore give exactly b).  The
row sum of d is a tree of depth k = D/256 + 8 (two adds per float4, at most eight float4 per lane, six shuffle levels):
|d mean| <= k u mean|x - x0| + u |mean - x0| (+ u |x - x0| per element when the subtraction rounds).  The second pass sums
(d - mean_d)^2 around the COMPUTED mean: relative variance error <= (k + 3) u + (d mean / sigma)^2, rstd = 1 / sqrtf(var + eps)
adds 2 ulp.  With r = 1 / sqrt(var + eps) in float64:
    |y - ref| <= |g| r (|d mean|max + u |x - x0| + |x - mean| ((k + 8) u + (|d mean|max r)^2)) + 4 u (|ref| + |b|)
followed by the output rounding of bf16 (2^-8 |out|) or e4m3 (2^-4 |out| + 2^-10).
"""
import numpy as np
import torch

U = 2.0 ** -24
LOG2E = 1.4426950408889634


def decode(t):
    """Operand or output tensor as the kernel stores it (bf16, float8_e4m3fn / e4m3 bytes as uint8, float32) -> float64."""
    if t.dtype == torch.uint8:
        t = t.view(torch.float8_e4m3fn)
    if t.dtype == torch.float8_e4m3fn:
        t = t.to(torch.float32)
    return t.to(torch.float64)


def attention_ref(qkv, T, heads, causal, img_chunk=None):
    """qkv [n*T, 3D] (any dtype, decoded to float64 on its device) -> (ref [n*T, D], absv [n*T, D] = a @ |v|, eps [n*T, D]) in
    float64; eps is the per-row eps_i of the module docstring broadcast over the head's 64 columns."""
    x = decode(qkv)
    rows, D3 = x.shape
    D = D3 // 3
    n = rows // T
    x = x.view(n, T, 3, heads, 64)
    ref = torch.empty((n, T, heads, 64), dtype=torch.float64, device=x.device)
    absv = torch.empty_like(ref)
    eps = torch.empty_like(ref)
    mask = torch.ones((T, T), dtype=torch.bool, device=x.device).tril() if causal else None
    step = img_chunk or max(1, int(2 ** 27 // max(1, heads * T * T)))
    for i0 in range(0, n, step):
        blk = x[i0:i0 + step]
        q, k, v = (blk[:, :, j].permute(0, 2, 1, 3) for j in range(3))      # [b, H, T, 64]
        s = q @ k.transpose(-1, -2)
        sa = q.abs() @ k.abs().transpose(-1, -2)
        if mask is not None:
            s = s.masked_fill(~mask, -np.inf)
            sa = sa.masked_fill(~mask, 0.0)
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        a = p / p.sum(-1, keepdim=True)
        span = torch.where(torch.isfinite(s), (s - m).abs(), torch.zeros_like(s)).amax(-1)
        e = 64 * U * sa.amax(-1) + 2 * U * span + 2 * U                   # [b, H, T]
        ref[i0:i0 + step] = (a @ v).permute(0, 2, 1, 3)
        absv[i0:i0 + step] = (a @ v.abs()).permute(0, 2, 1, 3)
        eps[i0:i0 + step] = e.permute(0, 2, 1)[..., None].expand(-1, -1, -1, 64)
    return ref.reshape(rows, D), absv.reshape(rows, D), eps.reshape(rows, D)


def attention_bound(ref, absv, eps, out_kind, T):
    """Per-element bound of |out - ref| (module docstring); out_kind 'bf16', 'e4m3' or 'f32'."""
    pre = (2.0 ** -8 + 2.0 ** -13 + 2 * eps) * absv + 4 * U * ref.abs()
    if out_kind == "bf16":
        return (1 + 2.0 ** -8) * pre + 2.0 ** -8 * ref.abs()
    if out_kind == "e4m3":
        return (1 + 2.0 ** -4) * pre + 2.0 ** -4 * ref.abs() + 2.0 ** -10
    if out_kind == "f32":
        return ((2 * T + 16) * U + 2 * eps) * absv + 4 * U * ref.abs()
    raise ValueError(out_kind)


def attention_error_ratio(out, qkv, T, heads, causal, out_kind):
    """max over elements of |out - ref| / bound (<= 1 passes), float."""
    ref, absv, eps = attention_ref(qkv, T, heads, causal)
    err = (decode(out).to(ref.device) - ref).abs()
    return float((err / attention_bound(ref, absv, eps, out_kind, T)).max())


def layernorm_ref(x, g, b, eps):
    """float64 LayerNorm of float32 rows x [R, D] -> (ref, r [R, 1], mean [R, 1]), two-pass statistics."""
    x, g, b = x.to(torch.float64), g.to(torch.float64), b.to(torch.float64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * r * g + b, r, mean


def layernorm_bound(x, g, b, eps, out_kind):
    """(ref, per-element bound of |out - ref|) for the float32 kernel followed by out_kind rounding ('f32', 'bf16', 'e4m3')."""
    ref, r, mean = layernorm_ref(x, g, b, eps)
    xd = x.to(torch.float64)
    D = x.shape[-1]
    k = D / 256 + 8
    dx = (xd - xd[:, :1]).abs()
    dmean = k * U * dx.mean(-1, keepdim=True) + U * (mean - xd[:, :1]).abs()
    gd, bd = g.to(torch.float64).abs(), b.to(torch.float64).abs()
    bound = gd * r * (dmean + U * dx + (xd - mean).abs() * ((k + 8) * U + (dmean * r) ** 2)) + 4 * U * (ref.abs() + bd)
    if out_kind == "bf16":
        bound = bound * (1 + 2.0 ** -8) + 2.0 ** -8 * ref.abs()
    elif out_kind == "e4m3":
        bound = bound * (1 + 2.0 ** -4) + 2.0 ** -4 * ref.abs() + 2.0 ** -10
    elif out_kind != "f32":
        raise ValueError(out_kind)
    return ref, bound


# ---- input designs shared by the CPU check of the bound and the GPU tests -------------------------------------------------------
# Each returns float32 numpy q, k, v [n, H, T, 64] whose values are exact in bf16 (and v exact in e4m3 where stated); pack() lays
# them out as the kernels' qkv rows.

def pack(q, k, v):
    """[n, H, T, 64] x3 -> qkv [n*T, 3*H*64] float32 (row = q | k | v, head h at columns h*64 of each part)."""
    n, H, T, _ = q.shape
    parts = [a.transpose(0, 2, 1, 3).reshape(n * T, H * 64) for a in (q, k, v)]
    return np.ascontiguousarray(np.concatenate(parts, axis=1), dtype=np.float32)


def unpack(att, n, T, H):
    """att [n*T, H*64] -> [n, H, T, 64]."""
    return np.asarray(att).reshape(n, T, H, 64).transpose(0, 2, 1, 3)


def design_uniform(rng, n, H, T):
    """Q = 0: every allowed key weighs the same, out = mean of V over the allowed keys.  V: integers in [-16, 16] (exact in e4m3)."""
    q = np.zeros((n, H, T, 64), np.float32)
    k = rng.integers(-4, 5, (n, H, T, 64)).astype(np.float32)
    v = rng.integers(-16, 17, (n, H, T, 64)).astype(np.float32)
    return q, k, v


def uniform_expected(v, causal):
    """float64 mean of V over the allowed keys: the full mean, or the prefix mean under the causal mask."""
    v = v.astype(np.float64)
    T = v.shape[2]
    if causal:
        return np.cumsum(v, axis=2) / np.arange(1, T + 1, dtype=np.float64)[:, None]
    return np.broadcast_to(v.mean(axis=2, keepdims=True), v.shape).copy()


def onehot_targets(T, causal, rng, edges=()):
    """pi(i): the key query i selects.  Hits key 0, key T-1, both sides of every 16 / 32 / 64-key block edge and of the given
    query-split edges; pi(i) <= i under the causal mask."""
    special = {0, T - 1}
    for blk in (16, 32, 64):
        for e in range(blk, T, blk):
            special.update((e - 1, e))
    for e in edges:
        special.update(x for x in (e - 1, e) if 0 <= x < T)
    special = np.array(sorted(special))
    pi = rng.integers(0, T, T)
    pi[rng.permutation(T)[:len(special)]] = special      # every special key is the target of some row
    if causal:
        pi = np.minimum(pi, np.arange(T))
        for key in special:                     # ... and, under the mask, of the row of the same index
            pi[key] = key
    return pi


def round_to(x, kind):
    """float64 numpy -> nearest value of the output dtype ('bf16', 'e4m3', 'f32'), as float64."""
    t = torch.from_numpy(np.asarray(x, np.float64))
    if kind == "e4m3":
        return t.clamp(-448, 448).to(torch.float8_e4m3fn).to(torch.float64).numpy()
    return t.to(torch.bfloat16 if kind == "bf16" else torch.float32).to(torch.float64).numpy()


def ulp(x, kind):
    """Spacing of the output dtype at |x| (the larger of the two binades at a power of two is NOT taken: callers pass the larger
    magnitude of the two values they compare)."""
    mant, emin = {"bf16": (7, -126), "e4m3": (3, -6), "f32": (23, -126)}[kind]
    _, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.ldexp(1.0, np.maximum(e - 1, emin) - mant)


def within_ulps(out, expected, kind, k=1):
    """|out - round(expected)| <= k ulps of the output dtype, elementwise (numpy bool array)."""
    r = round_to(expected, kind)
    out = np.asarray(out, np.float64)
    return np.abs(out - r) <= k * ulp(np.maximum(np.abs(r), np.abs(out)), kind)


def onehot_codes(rng, T):
    """T random +-1 codes of length 64 whose pairwise dot products are <= 40 (redrawn until they are)."""
    while True:
        c = rng.choice(np.array([-1.0, 1.0], np.float32), (T, 64))
        g = c @ c.T
        np.fill_diagonal(g, -64)
        if g.max() <= 40:
            return c


def onehot_values(rng, T):
    """V rows that are distinct non-zero integers, exact in bf16 and e4m3: key index in base 16 (+1) in columns 0..2, small integers
    elsewhere.  Non-zero, so that the off-target weights (<= e^-48 each) vanish in the output rounding."""
    v = rng.integers(1, 17, (T, 64)) * rng.choice([-1, 1], (T, 64))
    v = v.astype(np.float32)
    j = np.arange(T)
    v[:, 0], v[:, 1], v[:, 2] = j % 16 + 1, (j // 16) % 16 + 1, j // 256 + 1
    return v


def design_onehot(rng, n, H, T, causal, edges=()):
    """K_j = code_j, Q_i = 2 code_pi(i): the target's score 128 beats every other (<= 80) by >= 48 nats, so att[i] == V[pi(i)]."""
    q = np.empty((n, H, T, 64), np.float32)
    k = np.empty_like(q)
    v = np.empty_like(q)
    pis = np.empty((n, H, T), np.int64)
    for a in range(n):
        for h in range(H):
            c = onehot_codes(rng, T)
            pi = onehot_targets(T, causal, rng, edges)
            q[a, h], k[a, h], v[a, h] = 2 * c[pi], c, onehot_values(rng, T)
            pis[a, h] = pi
    return q, k, v, pis


def onehot_expected(v, pis):
    return np.take_along_axis(v, pis[..., None], axis=2)


def design_gaussian(rng, n, H, T, score_std, offset=0.0):
    """Gaussian Q, K with score standard deviation ~score_std, V standard normal; offset > 0 adds a common direction so that every
    score sits near `offset` (the max subtraction must carry it).  Values rounded to bf16."""
    a = np.sqrt(score_std / 8.0)
    q = rng.standard_normal((n, H, T, 64)) * a
    k = rng.standard_normal((n, H, T, 64)) * a
    if offset:
        u = rng.standard_normal((n, H, 1, 64))
        u /= np.linalg.norm(u, axis=-1, keepdims=True)
        q = q + u * np.sqrt(offset)
        k = k + u * np.sqrt(offset)
    v = rng.standard_normal((n, H, T, 64))
    r = lambda x: torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).to(torch.float32).numpy()   # noqa: E731
    return r(q), r(k), r(v)
