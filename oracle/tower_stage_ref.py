"""ORACLE (test infrastructure, never shipped, never imported by the product path).

Teacher-forced stage checks of an encoder tower (run_layers, run_pool, ivr_tower_encode_image / _text and ivr_tower_finalize in
csrc/tower.hip).  The tower's kernels are pinned one by one (gemm_ref, attention_ref); what composes them - strides, row subsets, the
aliased workspace, the dtype of every site - is pinned here.  Every stage's input and output are taken as the device held them
(ivr_tower_debug_capture), the float64 reference of that ONE kernel runs on the captured input, and the captured output has to sit
inside that kernel's per-element bound; whatever the stage must not write has to keep its bits.  No error is carried from stage to
stage, so no tolerance is added to the ones gemm_ref / attention_ref derive and tests/test_gemm_ref_cpu.py /
tests/test_attention_ref_cpu.py validate.  The one new bound is f_normalize's (below).

The weights are rebuilt here from the float32 master dict, independently of upload / upload_fp8 (device_weights):
  * the Q rows and the Q bias times head_dim ** -0.5 (0.125: exact), packed [q; k; v]
  * GEMM operands (patch_w, qkv_w, o_w, fc1_w, fc2_w, proj_w) rounded to bf16 (RNE) outside the f32 mode
  * sites at or past fp8_first_layer that are in the e4m3 mask: one scale per output row, s = amax / 448 (1 for a zero row), codes
    e4m3(w * (1 / s)) with every operation in float32.  quant_ref.quant_weight_e4m3 divides (w / s) where the device multiplies by
    the reciprocal; the two differ by one code on the few weights that land within an ulp of a rounding tie, which a per-element
    bound sees, so the device's order of operations is the one restated (the scales are quant_ref's to the bit).
    The MLP sites keep their bf16 copy next to the e4m3 one where token 0 takes the bf16 side path.
  * patch_w zero-padded to a multiple of 64 columns

Which rows a stage writes (n images of T tokens, B = max_batch; `pruned` = the last block of a vision tower under IVR_PRUNE_LAST):
  * full-size buffers: all n*T rows; the e4m3 fc2 with the side path leaves rows i*T (skip_mod = T)
  * pruned attn-out / fc2: rows i*T of the residual stream only (M = n, ldr = T*D); attn-out reads att rows i*T (unfused, att_ld =
    T*D) or the compact rows att[0, n) of the fused kernel
  * compact buffers (xn_cls, hid_cls, their e4m3 copy, pool, pooled_f32, eos_pos): rows [0, n) of B
The `before` image of a buffer is the last capture of the same workspace buffer earlier in program order: in the same call, or
else in the call before it on the same tower, which the tests make with other inputs and a full batch (n = B), so that the rows
behind the n written ones hold values a stray write would change.

f_normalize (f_normalize_kernel: one wave per row).  ss = sum x_k^2: a chain of d/64 fmas per lane (the square is exact inside the
fma, one rounding per link) and six shuffle levels of adds; every term is non-negative, so with one rounding taken as 2u relative
(u = 2^-24, the convention of gemm_ref) |ss_c - ss| <= 2 c u ss, c = d/64 + 6.  sqrtf is IEEE (2u), so the denominator is off by
(c + 2) u relative (the square root halves the error of ss), and one IEEE division adds 2u:
    |out - x / max(||x||, 1e-12f)| <= (c + 4) u |ref|
A zero row has ss = 0 exactly, the denominator is 1e-12f and the output 0 / 1e-12f = 0: the bound is 0 there, as the formula gives.
A row of norm below 1e-12f is divided by float32(1e-12) (one rounding: 2u |ref|, inside the bound); at the threshold both branches
agree to (c + 2) u.  normalize = 0 divides by 1.0f: x to the bit, bound 0.  tests/test_tower_stage_ref_cpu.py validates the bound the
way the others are (a float32 emulation stays inside with margin; the division without the floor leaves it).
"""
import math

import torch

from . import attention_ref as A
from . import gemm_ref as G

U = 2.0 ** -24
SITE_BITS = ("qkv", "o", "fc1", "fc2")
# stage kinds, in the order the summary prints them
KINDS = ("embed", "eos_pos", "pre_ln", "ln1", "qkv", "attention", "attn_out", "ln2", "ln2_cls", "fc1", "hid8", "fc2", "fc1_cls",
         "hid_cls8", "fc2_cls", "stream", "pool_ln", "proj", "f_normalize")


class Spec:
    """What a tower computes, from a TowerConfig and the Tower arguments (the presets of ivr_amd/tower.py restated)."""

    def __init__(self, cfg, compute="bf16", fp8_sites=None, fp8_cls_bf16=None, fp8_first_layer=None):
        self.cfg = cfg
        self.f32 = compute == "f32"
        self.fp8 = compute in ("fp8", "fp8_strict", "fp8_mlp", "fp8_all")
        self.sites, self.cls_bf16, self.first = frozenset(), False, 0
        if self.fp8:
            if fp8_sites is None:
                fp8_sites = SITE_BITS if compute == "fp8_all" else ("fc1", "fc2")
            self.sites = frozenset(fp8_sites)
            cls = (compute != "fp8_all") if fp8_cls_bf16 is None else bool(fp8_cls_bf16)
            self.cls_bf16 = cls and cfg.kind == "vision" and bool(self.sites & {"fc1", "fc2"})
            self.first = ((2 * cfg.layers) // 3 if compute in ("fp8", "fp8_strict") else 0) if fp8_first_layer is None else int(fp8_first_layer)
        self.base = "f32" if self.f32 else "bf16"
        self.kpad = -(-3 * cfg.patch * cfg.patch // 64) * 64 if cfg.kind == "vision" else 0

    def site8(self, layer, site):
        return self.fp8 and layer >= self.first and site in self.sites

    def side(self, layer):
        """the bf16 side path of token 0 runs in this block"""
        return self.cls_bf16 and (self.site8(layer, "fc1") or self.site8(layer, "fc2"))

    def kind(self, s8):
        """dtype of a GEMM A operand: LN output, attention output, MLP hidden"""
        return "f32" if self.f32 else "e4m3" if s8 else "bf16"


def _f32(a, dev):
    return torch.as_tensor(a, dtype=torch.float32).to(dev).contiguous()


def quant_rows_e4m3(w):
    """[N, K] float32 -> (e4m3 codes [N, K] float8_e4m3fn, scale [N] float32), the device's order of operations (module docstring)."""
    amax = w.abs().amax(dim=1, keepdim=True)
    s = torch.where(amax > 0, amax / torch.tensor(448.0, dtype=torch.float32, device=w.device), torch.ones_like(amax))
    inv = torch.ones_like(s) / s
    return (w * inv).clamp(-448.0, 448.0).to(torch.float8_e4m3fn), s.view(-1).contiguous()


def device_weights(spec, w, dev="cpu"):
    """The weights as the device holds them: {name: tensor}; GEMM weights under `name` (bf16 / float32) and / or `name@e4m3` +
    `name@scale`; everything else float32."""
    cfg, D = spec.cfg, spec.cfg.width
    op = (lambda t: t) if spec.f32 else (lambda t: t.to(torch.bfloat16))
    W = {}
    if cfg.kind == "vision":
        K = 3 * cfg.patch * cfg.patch
        pw = torch.zeros((D, spec.kpad), dtype=torch.float32, device=dev)
        pw[:, :K] = _f32(w["patch_w"], dev).view(D, K)
        W["patch_w"] = op(pw)
        for nme in ("patch_b",) * int(cfg.patch_bias) + ("cls",) + ("pre_ln_g", "pre_ln_b") * int(cfg.pre_ln):
            W[nme] = _f32(w[nme], dev).view(-1)
    else:
        W["tok"] = _f32(w["tok"], dev).view(cfg.vocab, D)
    W["pos"] = _f32(w["pos"], dev).view(cfg.tokens, D)
    scale = torch.tensor(float(D // cfg.heads) ** -0.5, dtype=torch.float32, device=dev)
    for i in range(cfg.layers):
        p = f"l{i}."
        m = {"qkv_w": torch.cat([_f32(w[p + "q_w"], dev).view(D, D) * scale, _f32(w[p + "k_w"], dev).view(D, D),
                                 _f32(w[p + "v_w"], dev).view(D, D)]),
             "o_w": _f32(w[p + "o_w"], dev).view(D, D), "fc1_w": _f32(w[p + "fc1_w"], dev).view(cfg.mlp, D),
             "fc2_w": _f32(w[p + "fc2_w"], dev).view(D, cfg.mlp)}
        for site, nme in zip(SITE_BITS, ("qkv_w", "o_w", "fc1_w", "fc2_w")):
            s8 = spec.site8(i, site)
            if s8:
                W[p + nme + "@e4m3"], W[p + nme + "@scale"] = quant_rows_e4m3(m[nme])
            if not s8 or (site in ("fc1", "fc2") and spec.cls_bf16):
                W[p + nme] = op(m[nme])
        W[p + "qkv_b"] = torch.cat([_f32(w[p + "q_b"], dev).view(-1) * scale, _f32(w[p + "k_b"], dev).view(-1), _f32(w[p + "v_b"], dev).view(-1)])
        for nme in ("ln1_g", "ln1_b", "ln2_g", "ln2_b", "o_b", "fc1_b", "fc2_b"):
            W[p + nme] = _f32(w[p + nme], dev).view(-1)
    W["post_ln_g"], W["post_ln_b"] = _f32(w["post_ln_g"], dev).view(-1), _f32(w["post_ln_b"], dev).view(-1)
    if cfg.out_dim:
        W["proj_w"] = op(_f32(w["proj_w"], dev).view(cfg.out_dim, D))
    return W


# ---- one function per stage: (ref, bound, written) over the whole captured output buffer `after` ---------------------------------
def _blank(after):
    z = torch.zeros(after.shape, dtype=torch.float64, device=after.device)
    return z, z.clone(), torch.zeros(after.shape, dtype=torch.bool, device=after.device)


def _gemm(spec, W, name, s8, before, x, *, epi, out_kind, N, K, act=-1, bias=None, **kw):
    """G.expect of one linear site: e4m3 operands with the per-row scale when the site runs in e4m3, else bf16 / float32."""
    if s8:
        return G.expect(before, x, W[name + "@e4m3"], dtype="e4m3", out_kind=out_kind, epi=epi, N=N, K=K, act=act, bias=bias,
                        colscale=W[name + "@scale"], **kw)
    return G.expect(before, x, W[name], dtype=spec.base, out_kind=out_kind, epi=epi, N=N, K=K, act=act, bias=bias, **kw)


def stage_vision_embed(spec, W, patches, before, n):
    """vision_cls_kernel + the patch GEMM's PATCH epilogue into the residual stream [n*T, D]: token-0 rows float32(cls + pos[0]) to
    the bit, patch row m at (m / G2) T + 1 + m % G2 with pos[1 + m % G2]."""
    cfg = spec.cfg
    T, G2, D = cfg.tokens, cfg.tokens - 1, cfg.width
    ref, bnd, written = G.expect(before, patches[:n * G2], W["patch_w"], dtype=spec.base, out_kind="f32", epi=G.PATCH, N=D, K=spec.kpad,
                                 bias=W.get("patch_b"), pos=W["pos"], T=T, G2=G2)
    ref[0::T] = (W["cls"] + W["pos"][0]).to(torch.float64)           # one float32 add
    bnd[0::T] = 0.0
    written[0::T] = True
    return ref, bnd, written


def stage_text_embed(spec, W, ids, after):
    """text_embed_kernel: float32(tok[clamp(id, 0, vocab - 1)] + pos[t]) to the bit."""
    cfg = spec.cfg
    q, T = ids.shape
    idc = ids.to(after.device).clamp(0, cfg.vocab - 1)
    ref, bnd, written = _blank(after)
    ref[:q * T] = (W["tok"][idc] + W["pos"][:T][None]).view(q * T, cfg.width).to(torch.float64)
    written[:q * T] = True
    return ref, bnd, written


def eos_positions(spec, ids):
    """first position of eos_id per row, 0 when absent (int64 [q])"""
    hit = ids == spec.cfg.eos_id
    T = ids.shape[1]
    first = torch.where(hit, torch.arange(T, device=ids.device)[None].expand_as(ids), torch.full_like(ids, T)).amin(1)
    return torch.where(first == T, torch.zeros_like(first), first)


def stage_eos_pos(spec, ids, after):
    ref, bnd, written = _blank(after)
    q = ids.shape[0]
    ref.view(-1)[:q] = eos_positions(spec, ids.to(after.device)).to(torch.float64)
    written.view(-1)[:q] = True
    return ref, bnd, written


def stage_layernorm(x, g, b, eps, out_kind, after):
    """layernorm_kernel on source rows x [R, D] (float32, already gathered) into rows [0, R) of the output buffer."""
    ref, bnd, written = _blank(after)
    R = x.shape[0]
    ref[:R], bnd[:R] = A.layernorm_bound(x, g, b, eps, out_kind)
    written[:R] = True
    return ref, bnd, written


def stage_attention(spec, qkv, T, out_kind, after):
    ref, absv, eps = A.attention_ref(qkv, T, spec.cfg.heads, bool(spec.cfg.causal))
    return ref, A.attention_bound(ref, absv, eps, out_kind, T), torch.ones(after.shape, dtype=torch.bool, device=after.device)


def stage_e4m3_copy(src, after, rows):
    """bf16_to_e4m3_kernel: rows [0, rows) of the copy equal the saturated RNE e4m3 of the bf16 rows, exactly."""
    ref, bnd, written = _blank(after)
    ref[:rows] = G.round_to(G.decode(src[:rows]), "e4m3")
    written[:rows] = True
    return ref, bnd, written


def stage_cls_resid(spec, W, name, s8, before, x, n, T, K, bias):
    """RESID GEMM of M = n rows into rows i*T of the residual stream [n*T, D] (ldr = T*D): every other row keeps its bits."""
    D = spec.cfg.width
    exp = _gemm(spec, W, name, s8, before[:n * T].reshape(n, T * D), x[:n], epi=G.RESID, out_kind="f32", N=D, K=K, bias=bias)
    return tuple(e.reshape(n * T, D) for e in exp)


def stage_f_normalize(x, normalize, after):
    """f_normalize_kernel on pooled rows x [n, d] float32 (module docstring)."""
    n, d = x.shape
    xd = x.to(torch.float64)
    ref, bnd, written = _blank(after)
    if normalize:
        den = torch.clamp(xd.pow(2).sum(1, keepdim=True).sqrt(), min=float(torch.tensor(1e-12, dtype=torch.float32)))
        ref[:n] = xd / den
        bnd[:n] = (d / 64 + 6 + 4) * U * ref[:n].abs()
    else:
        ref[:n] = xd
    written[:n] = True
    return ref, bnd, written


def raw(t):
    """the bytes of a tensor, flat"""
    return t.contiguous().view(-1).view(torch.uint8)


def verify(after, before, exp):
    """(largest |out - ref| / bound over the written elements - an exact stage (bound 0) gives 0 or inf -, number of bytes outside
    `written` that differ from `before`).  `before` may have another dtype or extent (the buffer's previous user): the bytes the
    two share are compared."""
    ref, bnd, written = exp
    err = (G.decode(after).to(ref.device) - ref).abs()
    inf = torch.full_like(err, math.inf)
    r = torch.where(bnd > 0, err / bnd, torch.where(err == 0, torch.zeros_like(err), inf))
    r = torch.where(torch.isnan(r), inf, r)[written]
    ratio = float(r.max()) if r.numel() else 0.0
    return ratio, changed_bytes(after, before, written)


def changed_bytes(after, before, written):
    """number of bytes of `after` outside `written` that differ from `before` (None: 0), over the bytes the two share"""
    if before is None:
        return 0
    a, b = raw(after), raw(before).to(after.device)
    keep = (~written).reshape(-1).repeat_interleave(after.element_size()).to(after.device)
    m = min(a.numel(), b.numel())
    return int(((a[:m] != b[:m]) & keep[:m]).sum())


# ---- the whole tower --------------------------------------------------------------------------------------------------------------
# the workspace buffer behind every capture site (tower.h)
BUFFER = {"embed": "resid", "stream": "resid", "attn_out": "resid", "fc2": "resid", "ln1": "xn", "ln2": "xn", "ln2_cls": "xn_cls",
          "qkv": "qkv", "att": "att", "hid": "hid", "hid8": "hid8", "hid_cls": "hid_cls", "hid_cls8": "hid_cls8", "eos_pos": "eos_pos",
          "pool_ln": "pool", "pooled": "pooled_f32"}


DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn, "i32": torch.int32}


def _z(after):
    """a `before` image for G.expect where the stage's unwritten elements are checked by bytes (verify) and not by value"""
    return torch.zeros(after.shape, dtype=torch.float32, device=after.device)


def capture_list(spec):
    """Every (layer, site) a call can produce, in program order."""
    cfg = spec.cfg
    out = [(0, "embed")] + ([(0, "eos_pos")] if cfg.kind == "text" else [])
    for i in range(cfg.layers):
        out += [(i, s) for s in ("stream", "ln1", "qkv", "att", "attn_out", "ln2", "ln2_cls", "hid", "hid8", "fc2", "hid_cls", "hid_cls8")]
    return out + [(cfg.layers, "stream"), (0, "pool_ln"), (0, "pooled")]


def _buffer_of(spec, key, pruned_last):
    layer, site = key
    if site == "ln2" and pruned_last and layer == spec.cfg.layers - 1:
        return "xn_cls"
    if site in ("pool_ln", "pooled") and spec.cfg.pool == 1:
        return "pooled_f32"
    return BUFFER[site]


class _Missing(Exception):
    pass


# the stage a capture site is the output of
STAGE_OF = {"embed": "embed", "eos_pos": "eos_pos", "stream": "stream", "ln1": "ln1", "qkv": "qkv", "att": "attention",
            "attn_out": "attn_out", "ln2": "ln2", "ln2_cls": "ln2_cls", "hid": "fc1", "hid8": "hid8", "hid_cls": "fc1_cls",
            "hid_cls8": "hid_cls8", "fc2": "fc2", "pool_ln": "pool_ln", "pooled": "proj"}


def check_tower(spec, W, caps, **kw):
    """Every stage of one captured call -> [(kind, layer, ratio, changed)] in program order.  caps: {(layer, site): tensor or None}
    for capture_list; keywords: n, T, pruned_last, out (the call's result [n, embed_dim]), normalize, patches / ids (its input) and
    prev_caps, the captures of the call before it on the same tower (same path): the `before` image of the buffers this call writes
    first.  A site the path should have materialised and did not ends the list with an infinite ratio at the stage that writes it."""
    res = []
    try:
        _check_tower(spec, W, caps, res, **kw)
    except _Missing as e:
        layer, site = e.args[0]
        res.append((STAGE_OF[site], layer, math.inf, 0))
    return res


def _check_tower(spec, W, caps, res, *, n, T, pruned_last, out, normalize, patches=None, ids=None, prev_caps=None):
    cfg, D, M = spec.cfg, spec.cfg.width, spec.cfg.mlp
    L = cfg.layers
    order = [k for k in capture_list(spec) if caps.get(k) is not None]
    porder = [k for k in capture_list(spec) if (prev_caps or {}).get(k) is not None]

    def before(key):
        """the last capture of the same workspace buffer earlier in program order, in this call or else the one before it"""
        buf, at = _buffer_of(spec, key, pruned_last), order.index(key)
        here = [k for k in order[:at] if _buffer_of(spec, k, pruned_last) == buf]
        if here:
            return caps[here[-1]]
        there = [k for k in porder if _buffer_of(spec, k, pruned_last) == buf]
        return prev_caps[there[-1]] if there else None

    def add(kind, layer, after, bef, exp, dt="f32"):
        if after.dtype != DTYPE[dt]:               # the site holds another dtype than the one its consumer reads
            res.append((kind, layer, math.inf, 0))
            return
        res.append((kind, layer) + verify(after, bef, exp))

    def same(kind, layer, a, b):
        res.append((kind, layer, 0.0 if torch.equal(raw(a), raw(b)) else math.inf, 0))

    def need(key):
        if caps.get(key) is None:
            raise _Missing(key)
        return caps[key]

    emb = need((0, "embed"))
    if cfg.kind == "vision":
        bef = before((0, "embed"))
        bef = bef[:n * T] if bef is not None and bef.shape[0] >= n * T else None
        add("embed", 0, emb, bef, stage_vision_embed(spec, W, patches, _z(emb) if bef is None else bef, n))
    else:
        add("embed", 0, emb, None, stage_text_embed(spec, W, ids, emb))
        add("eos_pos", 0, need((0, "eos_pos")), before((0, "eos_pos")), stage_eos_pos(spec, ids, caps[(0, "eos_pos")]), "i32")
    s0 = need((0, "stream"))
    if cfg.kind == "vision" and cfg.pre_ln:
        add("pre_ln", 0, s0, None, stage_layernorm(emb, W["pre_ln_g"], W["pre_ln_b"], cfg.ln_eps, "f32", s0))     # in place
    else:
        same("stream", 0, s0, emb)
    for i in range(L):
        p = f"l{i}."
        q8, o8, f18, f28 = (spec.site8(i, s) for s in SITE_BITS)
        side, last = spec.side(i), pruned_last and i == L - 1
        x_in = need((i, "stream"))
        ln1 = need((i, "ln1"))
        add("ln1", i, ln1, before((i, "ln1")), stage_layernorm(x_in, W[p + "ln1_g"], W[p + "ln1_b"], cfg.ln_eps, spec.kind(q8), ln1), spec.kind(q8))
        qkv, att = caps.get((i, "qkv")), need((i, "att"))
        fused = qkv is None
        if not fused:                 # the fused kernel keeps QKV in LDS: pinned by bit equality with the unfused run instead
            add("qkv", i, qkv, None, _gemm(spec, W, p + "qkv_w", q8, _z(qkv), ln1, epi=G.STORE, out_kind=spec.base, N=3 * D, K=D,
                                           bias=W[p + "qkv_b"]), spec.base)
            add("attention", i, att, None, stage_attention(spec, qkv, T, spec.kind(o8), att), spec.kind(o8))
        elif att.dtype != DTYPE[spec.kind(o8)]:
            res.append(("attention", i, math.inf, 0))
        elif last and before((i, "att")) is not None:      # pooled mode of the fused kernel: compact rows [0, n), the rest untouched
            wr = torch.zeros(att.shape, dtype=torch.bool, device=att.device)
            wr[:n] = True
            res.append(("attention", i, 0.0, changed_bytes(att, before((i, "att")), wr)))
        ao = need((i, "attn_out"))
        if last:
            xa = att[:n] if fused else att[0::T]
            add("attn_out", i, ao, x_in, stage_cls_resid(spec, W, p + "o_w", o8, x_in, xa, n, T, D, W[p + "o_b"]))
        else:
            add("attn_out", i, ao, x_in, _gemm(spec, W, p + "o_w", o8, x_in, att, epi=G.RESID, out_kind="f32", N=D, K=D, bias=W[p + "o_b"]))
        ln2 = need((i, "ln2"))
        s_out = need((i + 1, "stream"))
        c18, c28 = (f18 and not side, f28 and not side) if last else (f18, f28)
        hid_kind = "f32" if spec.f32 else "e4m3" if (c18 and c28) else "bf16"
        if last:
            add("ln2", i, ln2, before((i, "ln2")), stage_layernorm(ao[0::T], W[p + "ln2_g"], W[p + "ln2_b"], cfg.ln_eps, spec.kind(c18), ln2),
                spec.kind(c18))
            hc = need((i, "hid_cls"))
            add("fc1_cls", i, hc, before((i, "hid_cls")), _gemm(spec, W, p + "fc1_w", c18, _z(hc), ln2[:n], epi=G.STORE,
                                                                out_kind=hid_kind, N=M, K=D, act=cfg.act, bias=W[p + "fc1_b"]), hid_kind)
            xa = hc
            if c28 and not c18:
                xa = need((i, "hid_cls8"))
                add("hid_cls8", i, xa, before((i, "hid_cls8")), stage_e4m3_copy(hc, xa, n), "e4m3")
            add("fc2_cls", i, s_out, ao, stage_cls_resid(spec, W, p + "fc2_w", c28, ao, xa, n, T, M, W[p + "fc2_b"]))
            continue
        add("ln2", i, ln2, before((i, "ln2")), stage_layernorm(ao, W[p + "ln2_g"], W[p + "ln2_b"], cfg.ln_eps, spec.kind(f18), ln2),
            spec.kind(f18))
        hid = need((i, "hid"))
        add("fc1", i, hid, None, _gemm(spec, W, p + "fc1_w", f18, _z(hid), ln2, epi=G.STORE, out_kind=hid_kind, N=M, K=D,
                                       act=cfg.act, bias=W[p + "fc1_b"]), hid_kind)
        xa = hid
        if f28 and not f18:
            xa = need((i, "hid8"))
            add("hid8", i, xa, before((i, "hid8")), stage_e4m3_copy(hid, xa, n * T), "e4m3")
        fc2 = need((i, "fc2"))
        add("fc2", i, fc2, ao, _gemm(spec, W, p + "fc2_w", f28, ao, xa, epi=G.RESID, out_kind="f32", N=D, K=M, bias=W[p + "fc2_b"],
                                     skip_mod=T if side else 0))
        if not side:
            same("stream", i + 1, s_out, fc2)
            continue
        lc = need((i, "ln2_cls"))
        add("ln2_cls", i, lc, before((i, "ln2_cls")), stage_layernorm(ao[0::T], W[p + "ln2_g"], W[p + "ln2_b"], cfg.ln_eps, "bf16", lc), "bf16")
        hc = need((i, "hid_cls"))
        add("fc1_cls", i, hc, before((i, "hid_cls")), _gemm(spec, W, p + "fc1_w", False, _z(hc), lc[:n], epi=G.STORE,
                                                            out_kind="bf16", N=M, K=D, act=cfg.act, bias=W[p + "fc1_b"]), "bf16")
        add("fc2_cls", i, s_out, fc2, stage_cls_resid(spec, W, p + "fc2_w", False, fc2, hc, n, T, M, W[p + "fc2_b"]))
    final = need((L, "stream"))
    rows = torch.arange(n, device=final.device) * T
    if cfg.kind == "text":
        rows = rows + eos_positions(spec, ids.to(final.device))
    pl = need((0, "pool_ln"))
    pool_kind = "f32" if (spec.f32 or cfg.pool == 1) else "bf16"
    add("pool_ln", 0, pl, before((0, "pool_ln")), stage_layernorm(final[rows], W["post_ln_g"], W["post_ln_b"], cfg.ln_eps, pool_kind, pl), pool_kind)
    pooled = need((0, "pooled"))
    if cfg.pool == 1:
        same("proj", 0, pooled, pl)                  # no projection: f_normalize reads the LN rows
    else:
        add("proj", 0, pooled, before((0, "pooled")), G.expect(_z(pooled), pl[:n], W["proj_w"], dtype=spec.base, out_kind="f32",
                                                               epi=G.F32, N=cfg.out_dim, K=D))
    add("f_normalize", 0, out, None, stage_f_normalize(pooled[:n], normalize, out))


def worst(res):
    """{kind: (largest ratio, changed bytes)} over the records of check_tower, in KINDS order."""
    out = {}
    for kind, _, ratio, changed in res:
        r, c = out.get(kind, (0.0, 0))
        out[kind] = (max(r, ratio), c + changed)
    return {k: out[k] for k in KINDS if k in out}
