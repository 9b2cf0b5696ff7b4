"""CPU check of oracle/tower_stage_ref.py: an emulation of a correct tower - float32 arithmetic with the device's rounding points,
the device's row subsets and a byte-addressed workspace laid out as ivr_tower_finalize lays it out - passes every stage check with
margin on one tiny config per compute mode; the same emulation with one wiring fault fails at the stage that fault belongs to, by
ratio or by changed bits.  The kernels inside are the emulations the per-kernel oracles are validated with (test_gemm_ref_cpu.emulate,
test_attention_ref_cpu.emulate), so what is new here is the wiring between them."""
import numpy as np
import pytest
import torch

import test_attention_ref_cpu as AE
import test_gemm_ref_cpu as GE
from ivr_amd.config import ACT_GELU_ERF, POOL_EOS_LN_PROJ, POOL_LN_ALL_CLS, TowerConfig
from ivr_amd.weights import make_weights
from oracle import gemm_ref as G
from oracle import tower_stage_ref as S

f32 = GE.f32
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn}
ESZ = {"f32": 4, "bf16": 2, "e4m3": 1}


def rnd(v, kind):
    v = f32(v)
    return GE.to_bf16(v) if kind == "bf16" else GE.to_e4m3(v) if kind == "e4m3" else v


def val(t):
    """typed torch tensor -> float32 numpy values"""
    return t.to(torch.float32).numpy()


def layernorm(x, g, b, eps):
    """layernorm_kernel in float32: two-pass statistics on d = x - x[0]"""
    x = f32(x)
    D = np.float32(x.shape[1])
    d = x - x[:, :1]
    mean = f32(d.sum(1, dtype=np.float32, keepdims=True) / D)
    c = f32(d - mean)
    var = f32((c * c).sum(1, dtype=np.float32, keepdims=True) / D)
    rstd = f32(np.float32(1) / np.sqrt(f32(var + np.float32(eps))))
    return f32(f32(c * rstd) * g + b)


def act_f32(v, act):
    """act_fn<false>: the float32 mode's activation"""
    v = f32(v)
    if act == G.QUICK:
        return f32(v / f32(np.float32(1) + np.exp(f32(np.float32(-1.702) * v))))
    return f32(np.float32(0.5) * v * f32(np.float32(1) + torch.erf(torch.from_numpy(f32(v * np.float32(0.70710678)))).numpy()))


class EmuTower:
    """A tower on a byte-addressed workspace.  `spec` is what the emulated tower DOES (a fault may give it another fp8_first_layer
    than the checker expects); faults: a set of names (FAULTS below)."""

    def __init__(self, spec, w, max_batch, faults=()):
        self.spec, self.cfg, self.B, self.faults = spec, spec.cfg, max_batch, frozenset(faults)
        cfg, B = spec.cfg, max_batch
        w = {k: np.array(v, copy=True) for k, v in w.items()}
        for i in range(cfg.layers):
            p = f"l{i}."
            if "q_scale_missing" in self.faults:
                w[p + "q_w"] *= 8
                w[p + "q_b"] *= 8
            if "q_scale_twice" in self.faults:
                w[p + "q_w"] /= 8
                w[p + "q_b"] /= 8
            if "k_bias_in_q" in self.faults:
                w[p + "q_b"] = w[p + "k_b"] * 8
        self.W = S.device_weights(spec, w)
        D, M, Tk = cfg.width, cfg.mlp, cfg.tokens
        es = 4 if spec.f32 else 2
        z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8)      # noqa: E731
        self.ws = {"resid": z(B * Tk * D * 4), "xn": z(B * Tk * D * es), "qkv": z(B * Tk * 3 * D * es), "att": z(B * Tk * D * es),
                   "hid": z(B * Tk * M * (es + 1)), "pool": z(B * D * es), "pooled_f32": z(B * max(D, cfg.out_dim) * 4), "eos_pos": z(B * 4),
                   "xn_cls": z(B * D * es), "hid_cls": z(B * M * (es + 1))}

    def view(self, name, kind, rows, cols, off=0):
        dt = torch.int32 if kind == "i32" else TDT[kind]
        nbytes = rows * cols * (4 if kind == "i32" else ESZ[kind])
        return self.ws[name][off:off + nbytes].view(dt).view(rows, cols)

    def put(self, name, kind, rows_idx, values, cols, off=0, nrows=None):
        """write float32 values into rows rows_idx of the typed view"""
        v = self.view(name, kind, nrows, cols, off)
        v[rows_idx] = torch.from_numpy(f32(values)).to(v.dtype)

    def wv(self, name, s8):
        """GEMM weight values, colscale"""
        if s8:
            return val(self.W[name + "@e4m3"]), self.W[name + "@scale"].numpy()
        return val(self.W[name]), None

    def gemm_store(self, x, name, s8, out_kind, act=-1, bias=None):
        wv, cs = self.wv(name, s8)
        dt = "e4m3" if s8 else self.spec.base
        before = np.zeros((x.shape[0], wv.shape[0]), np.float32)
        if self.spec.f32 and act >= 0:
            return act_f32(GE.emulate(before, x, wv, dtype=dt, out_kind="f32", epi=G.STORE, bias=bias, colscale=cs), act)
        return GE.emulate(before, x, wv, dtype=dt, out_kind=out_kind, epi=G.STORE, act=act, bias=bias, colscale=cs)

    def gemm_resid(self, before, x, name, s8, bias, skip_mod=0):
        wv, cs = self.wv(name, s8)
        return GE.emulate(before, x, wv, dtype="e4m3" if s8 else self.spec.base, out_kind="f32", epi=G.RESID, bias=bias, colscale=cs,
                          skip_mod=skip_mod)

    def run(self, *, n, T, prune, fused, normalize, patches=None, ids=None):
        """one encode call -> (out [n, E] float32 tensor, caps)"""
        spec, cfg, W, B, F = self.spec, self.cfg, self.W, self.B, self.faults
        D, M, L, Tk = cfg.width, cfg.mlp, cfg.layers, cfg.tokens
        R = n * T
        caps = {}
        cap = lambda key, name, kind, rows, cols, off=0: caps.__setitem__(key, self.view(name, kind, rows, cols, off).clone())   # noqa: E731
        resid = self.view("resid", "f32", R, D)
        if cfg.kind == "vision":
            G2 = T - 1
            pos = W["pos"].numpy()
            resid[0::T] = torch.from_numpy(f32(W["cls"].numpy() + pos[0]))
            fault = "pos_off_by_one" if "pos_off_by_one" in F else "token0_written" if "token0_written" in F else None
            pb = W["patch_b"].numpy() if cfg.patch_bias else None
            resid[:] = torch.from_numpy(GE.emulate(resid.numpy().copy(), val(patches[:n * G2]), val(W["patch_w"]), dtype=spec.base,
                                                   out_kind="f32", epi=G.PATCH, bias=pb, pos=pos, T=T, G2=G2, fault=fault))
            cap((0, "embed"), "resid", "f32", R, D)
            if cfg.pre_ln and "pre_ln_skipped" not in F:
                resid[:] = torch.from_numpy(layernorm(resid.numpy(), W["pre_ln_g"].numpy(), W["pre_ln_b"].numpy(), cfg.ln_eps))
        else:
            idc = ids.clamp(0, cfg.vocab - 1)
            resid[:] = (W["tok"][idc] + W["pos"][:T][None]).view(R, D)
            hit = (ids == cfg.eos_id).numpy()
            ep = np.array([(np.nonzero(h)[0][-1 if "last_eos" in F else 0] if h.any() else 0) for h in hit], np.int32)
            self.view("eos_pos", "i32", B, 1)[:n, 0] = torch.from_numpy(ep)
            cap((0, "embed"), "resid", "f32", R, D)
            cap((0, "eos_pos"), "eos_pos", "i32", B, 1)
            prune = False
        es = spec.base
        for i in range(L):
            p = f"l{i}."
            q8, o8, f18, f28 = (spec.site8(i, s) for s in S.SITE_BITS)
            side, last = spec.side(i), prune and i == L - 1
            cap((i, "stream"), "resid", "f32", R, D)
            k1 = spec.kind(q8)
            self.put("xn", k1, slice(0, R), rnd(layernorm(resid.numpy(), W[p + "ln1_g"].numpy(), W[p + "ln1_b"].numpy(), cfg.ln_eps), k1), D, nrows=R)
            cap((i, "ln1"), "xn", k1, R, D)
            xn = val(self.view("xn", k1, R, D))
            ko = spec.kind(o8)
            qkv = self.gemm_store(xn, p + "qkv_w", q8, es, bias=W[p + "qkv_b"].numpy())
            if not fused:
                self.put("qkv", es, slice(0, R), qkv, 3 * D, nrows=R)
                cap((i, "qkv"), "qkv", es, R, 3 * D)
            else:
                caps[(i, "qkv")] = None
            x5 = f32(qkv).reshape(n, T, 3, cfg.heads, 64)
            qq, kk, vv = (np.ascontiguousarray(x5[:, :, j].transpose(0, 2, 1, 3)) for j in range(3))
            with np.errstate(all="ignore"):                  # a fault upstream may have fed NaN
                att = AE.emulate(qq, kk, vv, bool(cfg.causal), ko).transpose(0, 2, 1, 3).reshape(R, D)
            if fused and last:
                self.put("att", ko, slice(0, n), att[0::T], D, nrows=R)          # compact rows of query 0
            else:
                self.put("att", ko, slice(0, R), att, D, nrows=R)
            cap((i, "att"), "att", ko, R, D)
            attv = val(self.view("att", ko, R, D))
            ob = W[p + "o_b"].numpy()
            if last:
                xa = attv[:n] if fused else (attv[:n] if "prune_att_stride_D" in F else attv[0::T])
                if "prune_attn_out_row_i" in F:
                    resid[:n] = torch.from_numpy(self.gemm_resid(resid[:n].numpy().copy(), xa, p + "o_w", o8, ob))
                else:
                    r2 = resid.numpy().reshape(n, T * D).copy()
                    resid[:] = torch.from_numpy(self.gemm_resid(r2, xa, p + "o_w", o8, ob).reshape(R, D))
            else:
                resid[:] = torch.from_numpy(self.gemm_resid(resid.numpy().copy(), attv, p + "o_w", o8, ob))
            cap((i, "attn_out"), "resid", "f32", R, D)
            g2, b2 = W[p + "ln2_g"].numpy(), W[p + "ln2_b"].numpy()
            f1b, f2b = W[p + "fc1_b"].numpy(), W[p + "fc2_b"].numpy()
            for s in ("ln2_cls", "hid", "hid8", "fc2", "hid_cls", "hid_cls8"):
                caps[(i, s)] = None
            if last:
                c18, c28 = f18 and not side, f28 and not side
                kc = spec.kind(c18)
                self.put("xn_cls", kc, slice(0, n), rnd(layernorm(resid.numpy()[0::T], g2, b2, cfg.ln_eps), kc), D, nrows=B)
                cap((i, "ln2"), "xn_cls", kc, B, D)
                hk = "f32" if spec.f32 else "e4m3" if (c18 and c28) else "bf16"
                h = self.gemm_store(val(self.view("xn_cls", kc, n, D)), p + "fc1_w", c18, hk, act=cfg.act, bias=f1b)
                self.put("hid_cls", hk, slice(0, n), h, M, nrows=B)
                cap((i, "hid_cls"), "hid_cls", hk, B, M)
                ha = val(self.view("hid_cls", hk, n, M))
                if c28 and not c18:
                    self.put("hid_cls", "e4m3", slice(0, n), GE.to_e4m3(ha), M, off=B * M * 2, nrows=B)
                    cap((i, "hid_cls8"), "hid_cls", "e4m3", B, M, B * M * 2)
                    ha = val(self.view("hid_cls", "e4m3", n, M, B * M * 2))
                if "prune_fc2_row_i" in F:
                    resid[:n] = torch.from_numpy(self.gemm_resid(resid[:n].numpy().copy(), ha, p + "fc2_w", c28, f2b))
                else:
                    r2 = resid.numpy().reshape(n, T * D).copy()
                    resid[:] = torch.from_numpy(self.gemm_resid(r2, ha, p + "fc2_w", c28, f2b).reshape(R, D))
                continue
            k2 = spec.kind(f18)
            y = rnd(layernorm(resid.numpy(), g2, b2, cfg.ln_eps), k2)
            if "ln_bf16_for_e4m3" in F and k2 == "e4m3":
                self.put("xn", "bf16", slice(0, R), GE.to_bf16(layernorm(resid.numpy(), g2, b2, cfg.ln_eps)), D, nrows=R)
            else:
                self.put("xn", k2, slice(0, R), y, D, nrows=R)
            cap((i, "ln2"), "xn", k2, R, D)
            if side:
                src = resid.numpy()[:n] if "side_ln2_rows_i" in F else resid.numpy()[0::T]
                self.put("xn_cls", "bf16", slice(0, n), GE.to_bf16(layernorm(src, g2, b2, cfg.ln_eps)), D, nrows=B)
                cap((i, "ln2_cls"), "xn_cls", "bf16", B, D)
            hk = "f32" if spec.f32 else "e4m3" if (f18 and f28) else "bf16"
            h = self.gemm_store(val(self.view("xn", k2, R, D)), p + "fc1_w", f18, hk, act=cfg.act, bias=f1b)
            self.put("hid", hk, slice(0, R), h, M, nrows=R)
            cap((i, "hid"), "hid", hk, R, M)
            ha = val(self.view("hid", hk, R, M))
            if f28 and not f18:
                off = (n if "hid8_offset_n" in F else B) * Tk * M * 2
                if not ("stale_hid8" in F and i > spec.first):
                    self.put("hid", "e4m3", slice(0, R), GE.to_e4m3(ha), M, off=off, nrows=R)
                cap((i, "hid8"), "hid", "e4m3", R, M, B * Tk * M * 2)
                ha = val(self.view("hid", "e4m3", R, M, off))
            skip = T if (side and "no_skip_mod" not in F) else 0
            resid[:] = torch.from_numpy(self.gemm_resid(resid.numpy().copy(), ha, p + "fc2_w", f28, f2b, skip_mod=skip))
            cap((i, "fc2"), "resid", "f32", R, D)
            if side and "side_skipped" not in F:
                h = self.gemm_store(val(self.view("xn_cls", "bf16", n, D)), p + "fc1_w", False, "bf16", act=cfg.act, bias=f1b)
                self.put("hid_cls", "bf16", slice(0, n), h, M, nrows=B)
                cap((i, "hid_cls"), "hid_cls", "bf16", B, M)
                r2 = resid.numpy().reshape(n, T * D).copy()
                resid[:] = torch.from_numpy(self.gemm_resid(r2, val(self.view("hid_cls", "bf16", n, M)), p + "fc2_w", False, f2b).reshape(R, D))
            elif side:
                cap((i, "hid_cls"), "hid_cls", "bf16", B, M)
        cap((L, "stream"), "resid", "f32", R, D)
        rows = np.arange(n) * T
        if cfg.kind == "text":
            rows = rows + self.view("eos_pos", "i32", B, 1)[:n, 0].numpy()
        if "pool_neighbour" in F:
            rows = np.roll(rows, 1)
        y = layernorm(resid.numpy()[rows], W["post_ln_g"].numpy(), W["post_ln_b"].numpy(), cfg.ln_eps)
        if cfg.pool == POOL_LN_ALL_CLS:
            self.put("pooled_f32", "f32", slice(0, n), y, D, nrows=B)
            cap((0, "pool_ln"), "pooled_f32", "f32", B, D)
            cap((0, "pooled"), "pooled_f32", "f32", B, D)
            E = D
        else:
            self.put("pool", es, slice(0, n), rnd(y, es), D, nrows=B)
            cap((0, "pool_ln"), "pool", es, B, D)
            E = cfg.out_dim
            wv = val(W["proj_w"])
            pr = GE.emulate(np.zeros((n, E), np.float32), val(self.view("pool", es, n, D)), wv, dtype=es, out_kind="f32", epi=G.F32)
            self.put("pooled_f32", "f32", slice(0, n), pr, E, nrows=B)
            cap((0, "pooled"), "pooled_f32", "f32", B, E)
        x = self.view("pooled_f32", "f32", n, E).numpy()
        if normalize:
            ss = (x * x).sum(1, dtype=np.float32, keepdims=True)
            with np.errstate(invalid="ignore", divide="ignore"):
                den = np.sqrt(ss) if "no_floor" in F else np.maximum(np.sqrt(ss), np.float32(1e-12))
                out = f32(x / den)
        else:
            out = x.copy()
        return torch.from_numpy(out), caps


def vision_cfg(**kw):
    base = dict(name="emu-vit", kind="vision", width=128, layers=3, heads=2, mlp=256, tokens=5, out_dim=64, image=8, patch=4)
    base.update(kw)
    return TowerConfig(**base)


TEXT = TowerConfig("emu-text", "text", 128, 2, 2, 256, 12, 64, pool=POOL_EOS_LN_PROJ, vocab=64, eos_id=63, causal=True)
# compute, Tower arguments
MODES = {"f32": ("f32", {}), "bf16": ("bf16", {}), "fp8": ("fp8", {}), "fp8_mlp": ("fp8_mlp", {}), "fp8_all": ("fp8_all", {}),
         "fp8_all_o": ("fp8_all", {"fp8_sites": ("o",)}), "fp8_all_fc2": ("fp8_all", {"fp8_sites": ("fc2",)}),
         "fp8_fc2_side": ("fp8_mlp", {"fp8_sites": ("fc2",)})}


def patches_for(cfg, spec, rng, n):
    kpad, K = spec.kpad, 3 * cfg.patch * cfg.patch
    x = np.zeros((n * (cfg.tokens - 1), kpad), np.float32)
    x[:, :K] = rng.standard_normal((x.shape[0], K))
    return torch.from_numpy(x) if spec.f32 else torch.from_numpy(x).to(torch.bfloat16)


def text_ids(cfg, rng, q, T):
    """first EOS at 0, at T-1, in the middle with more behind it, absent; an id below 0 and one >= vocab"""
    ids = rng.integers(1, cfg.vocab - 1, (q, T))
    ids[0, 0] = cfg.eos_id
    ids[1, T - 1] = cfg.eos_id
    ids[2, T // 2] = ids[2, T // 2 + 2] = ids[2, T - 1] = cfg.eos_id
    ids[3, 1], ids[3, 2] = -5, cfg.vocab + 7
    return torch.from_numpy(ids.astype(np.int64))


def run_case(cfg, mode, *, n=3, prune=True, fused=False, faults=(), normalize=True, emu_first_layer=None, wmod=None, T=None):
    compute, kw = MODES[mode]
    spec = S.Spec(cfg, compute, **kw)
    emu_spec = spec if emu_first_layer is None else S.Spec(cfg, compute, **dict(kw, fp8_first_layer=emu_first_layer))
    w = make_weights(cfg, 5)
    if wmod:
        wmod(w)
    B = 2 * n + 3
    T = T or cfg.tokens
    tw = EmuTower(emu_spec, w, B, faults)
    rng = np.random.default_rng(17)
    if cfg.kind == "vision":
        prev_in, cur_in = dict(patches=patches_for(cfg, spec, rng, B)), dict(patches=patches_for(cfg, spec, rng, n))
    else:
        prev_in, cur_in = dict(ids=torch.from_numpy(rng.integers(0, cfg.vocab, (B, T)))), dict(ids=text_ids(cfg, rng, n, T))
    _, prev = tw.run(n=B, T=T, prune=prune, fused=fused, normalize=normalize, **prev_in)
    out, caps = tw.run(n=n, T=T, prune=prune, fused=fused, normalize=normalize, **cur_in)
    W = S.device_weights(spec, w)
    return S.check_tower(spec, W, caps, n=n, T=T, pruned_last=prune and cfg.kind == "vision", out=out, normalize=normalize,
                         prev_caps=prev, **cur_in)


def failing(res):
    return sorted({kind for kind, _, ratio, changed in res if not ratio <= 1.0 or changed})


# the fused kernel takes bf16 QKV sites only
CORRECT = [(m, p, False) for m in MODES for p in (True, False)] + [(m, p, True) for m in MODES if m not in ("f32", "fp8_all") for p in (True, False)]


@pytest.mark.parametrize("mode,prune,fused", CORRECT)
def test_correct_tower_passes_every_stage(mode, prune, fused):
    res = run_case(vision_cfg(), mode, prune=prune, fused=fused)
    worst = S.worst(res)
    print(mode, "prune" if prune else "full", "fused" if fused else "", {k: round(v[0], 3) for k, v in worst.items()})
    assert failing(res) == [], [r for r in res if not r[2] <= 1.0 or r[3]]
    assert all(v[0] < 1.0 for v in worst.values())


def test_correct_dino_shape_and_text_tower_pass():
    dino = vision_cfg(act=ACT_GELU_ERF, pool=POOL_LN_ALL_CLS, pre_ln=False, patch_bias=True, out_dim=0, ln_eps=1e-12)
    for cfg, mode, kw in ((dino, "bf16", {}), (dino, "f32", {}), (TEXT, "bf16", dict(n=4)), (TEXT, "f32", dict(n=4, T=7)),
                          (TEXT, "bf16", dict(n=4, normalize=False))):
        res = run_case(cfg, mode, **kw)
        print(cfg.name, mode, {k: round(v[0], 3) for k, v in S.worst(res).items()})
        assert failing(res) == [], [r for r in res if not r[2] <= 1.0 or r[3]]
        assert all(v[0] < 1.0 for v in S.worst(res).values())


def zero_post_ln(w):
    w["post_ln_g"][:] = 0
    w["post_ln_b"][:] = 0


def tiny_post_ln(w):
    w["post_ln_g"] *= np.float32(1e-14)
    w["post_ln_b"] *= np.float32(1e-14)


@pytest.mark.parametrize("wmod", [zero_post_ln, tiny_post_ln])
def test_f_normalize_edge_rows(wmod):
    """zero rows (0 / 1e-12 = 0 exactly) and rows of norm below 1e-12 (divided by 1e-12f); without the floor both leave the bound"""
    res = run_case(vision_cfg(), "bf16", wmod=wmod)
    assert failing(res) == [], res
    assert "f_normalize" in failing(run_case(vision_cfg(), "bf16", wmod=wmod, faults=("no_floor",)))


# fault, mode, run_case arguments, the stage kinds of which at least one must fail (and no EARLIER stage of another kind may)
FAULTS = [
    ("prune_attn_out_row_i", "bf16", {}, {"attn_out"}),
    ("prune_fc2_row_i", "bf16", {}, {"fc2_cls"}),
    ("prune_fc2_row_i", "fp8_all_fc2", {}, {"fc2_cls"}),
    ("prune_att_stride_D", "bf16", {}, {"attn_out"}),
    ("no_skip_mod", "fp8_mlp", {}, {"fc2"}),
    ("side_skipped", "fp8_mlp", {}, {"fc1_cls", "fc2_cls"}),
    ("side_ln2_rows_i", "fp8_mlp", {}, {"ln2_cls"}),
    ("stale_hid8", "fp8_all_fc2", {}, {"hid8"}),
    ("hid8_offset_n", "fp8_all_fc2", {}, {"hid8"}),
    ("q_scale_missing", "bf16", {}, {"qkv"}),
    ("q_scale_twice", "fp8_all", {}, {"qkv"}),
    ("k_bias_in_q", "bf16", {}, {"qkv"}),
    ("pos_off_by_one", "bf16", {}, {"embed"}),
    ("token0_written", "f32", {}, {"embed"}),
    ("pre_ln_skipped", "bf16", {}, {"pre_ln"}),
    ("last_eos", "bf16", {"text": True}, {"eos_pos"}),
    ("pool_neighbour", "bf16", {}, {"pool_ln"}),
    ("pool_neighbour", "bf16", {"text": True}, {"pool_ln"}),
    ("ln_bf16_for_e4m3", "fp8_mlp", {}, {"ln2"}),
    ("fp8_first_layer_off_by_one", "fp8", {"prune": False}, {"ln2"}),
    ("no_floor", "bf16", {"wmod": tiny_post_ln}, {"f_normalize"}),
]


@pytest.mark.parametrize("fault,mode,kw,stages", FAULTS, ids=[f"{f[0]}-{f[1]}" + ("-text" if f[2].get("text") else "") for f in FAULTS])
def test_wiring_fault_fails_at_its_stage(fault, mode, kw, stages):
    kw = dict(kw)
    cfg = TEXT if kw.pop("text", False) else vision_cfg()
    if cfg is TEXT:
        kw["n"] = 4
    if fault == "fp8_first_layer_off_by_one":
        res = run_case(cfg, mode, emu_first_layer=S.Spec(cfg, "fp8").first + 1, **kw)
    else:
        res = run_case(cfg, mode, faults=(fault,), **kw)
    bad = failing(res)
    print(fault, mode, "->", bad)
    assert stages & set(bad), (fault, bad)
    first_bad = next(kind for kind, _, ratio, changed in res if not ratio <= 1.0 or changed)
    assert first_bad in stages, (fault, first_bad, bad)       # teacher forcing: nothing upstream of the fault is blamed


def test_weight_restatement_matches_quant_ref_scales():
    """the e4m3 scales are quant_ref's to the bit; the codes differ from its w / s on at most a few rounding ties"""
    from oracle import quant_ref as Q
    w = torch.from_numpy(np.random.default_rng(3).standard_normal((384, 192)).astype(np.float32))
    w[7] = 0
    codes, s = S.quant_rows_e4m3(w)
    qv, qs = Q.quant_weight_e4m3(w)
    assert torch.equal(s, qs.view(-1))
    assert (codes.to(torch.float32) != qv).float().mean() < 1e-4
