"""GPU: every stage of an encoder tower per element against float64 (oracle/tower_stage_ref.py).

Each test makes two encode calls on one tower with every capture site armed (ivr_tower_debug_capture): a full batch (n = max_batch)
of other inputs, then the call under test with n < max_batch = 2n + 3.  For every block and every stage of the second call the
float64 reference of that one kernel runs on the captured input; the captured output has to sit inside the kernel's derived bound
(ratio <= 1), and every byte the stage must not write has to equal the buffer's previous capture.  The largest ratio per stage kind
is printed.  The bounds are gemm_ref's, attention_ref's and the f_normalize bound derived in tower_stage_ref; none is set here.

Shapes: width 192 (3 heads, the narrowest the fused QKV + attention kernel takes), mlp 384, 3 layers; the e4m3 presets at width 256,
because ivr_tower_create takes the fp8 mode at multiples of 128 only.  Tokens 10 and 50 (2 to 25 images per 256-row tile of the
fused kernel), 65 (first length past it), 197 at width 384 with GELU, a patch bias, no pre-LN and LN_ALL_CLS pooling.  n = 1, 5, 23:
n*T ragged against 128- and 256-row tiles."""
import numpy as np
import pytest
import torch

from ivr_amd.config import ACT_GELU_ERF, POOL_EOS_LN_PROJ, POOL_LN_ALL_CLS, TowerConfig
from ivr_amd.weights import make_weights
from oracle import tower_stage_ref as S

pytestmark = pytest.mark.gpu

# compute, Tower arguments
MODES = {"f32": ("f32", {}), "bf16": ("bf16", {}), "fp8": ("fp8", {"fp8_first_layer": 2}), "fp8_mlp": ("fp8_mlp", {}),
         "fp8_all": ("fp8_all", {}), "fp8_all_o": ("fp8_all", {"fp8_sites": ("o",)}), "fp8_all_fc2": ("fp8_all", {"fp8_sites": ("fc2",)})}


def vision_cfg(T, mode):
    grid = {10: 3, 50: 7, 65: 8, 197: 14}[T]
    if T == 197:
        return TowerConfig("stage-vit-197", "vision", 384, 3, 6, 768, T, 0, act=ACT_GELU_ERF, ln_eps=1e-12, pool=POOL_LN_ALL_CLS,
                           image=4 * grid, patch=4, pre_ln=False, patch_bias=True)
    width = 256 if mode.startswith("fp8") else 192
    return TowerConfig(f"stage-vit-{T}-{width}", "vision", width, 3, width // 64, 384, T, 64, image=4 * grid, patch=4)


TEXT = TowerConfig("stage-text", "text", 128, 2, 2, 256, 77, 64, pool=POOL_EOS_LN_PROJ, vocab=512, eos_id=511, causal=True)


def patches_for(cfg, spec, seed, n):
    K = 3 * cfg.patch * cfg.patch
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros((n * (cfg.tokens - 1), spec.kpad))
    x[:, :K] = torch.randn((x.shape[0], K), generator=g)
    return x.to(torch.float32 if spec.f32 else torch.bfloat16).cuda()


def capture_run(cfg, mode, n, *, normalize=True, wmod=None, ids=None, prev_ids=None):
    """(spec, device weights, captures of the call under test, captures of the call before it, out, input)"""
    from ivr_amd.tower import Tower
    compute, kw = MODES[mode]
    spec = S.Spec(cfg, compute, **kw)
    w = make_weights(cfg, 5)
    if wmod:
        wmod(w)
    B = 2 * n + 3
    tw = Tower(cfg, w, max_batch=B, compute=compute, **kw)
    keys = S.capture_list(spec)
    if cfg.kind == "vision":
        x = patches_for(cfg, spec, 100 + n, n)
        _, prev = tw.encode_patches(patches_for(cfg, spec, 7, B), B, normalize=normalize, capture=keys)
        out, caps = tw.encode_patches(x, n, normalize=normalize, capture=keys)
    else:
        x = ids.cuda()
        _, prev = tw.encode_ids(prev_ids, normalize=normalize, capture=keys)
        out, caps = tw.encode_ids(x, normalize=normalize, capture=keys)
    torch.cuda.synchronize()
    return spec, S.device_weights(spec, w, "cuda"), caps, prev, out, x


def check(res, label):
    worst = S.worst(res)
    print(label, " ".join(f"{k}={v[0]:.3f}" + (f"(!{v[1]} bytes)" if v[1] else "") for k, v in worst.items()))
    bad = [r for r in res if not r[2] <= 1.0 or r[3]]
    assert not bad, bad


# (tokens, n, mode, prune): every value of every axis occurs; every e4m3 preset with both prune settings and with n = 1 and n = 23
VISION = [(10, 5, "f32", 1), (65, 1, "f32", 0), (50, 23, "bf16", 1), (10, 1, "bf16", 0), (65, 5, "bf16", 1), (197, 5, "bf16", 1),
          (197, 1, "f32", 0),
          (50, 1, "fp8", 1), (10, 23, "fp8", 0), (10, 23, "fp8_mlp", 1), (65, 1, "fp8_mlp", 0), (65, 23, "fp8_all", 1),
          (50, 1, "fp8_all", 0), (50, 23, "fp8_all_o", 1), (10, 1, "fp8_all_o", 0), (10, 1, "fp8_all_fc2", 1), (50, 23, "fp8_all_fc2", 0)]


@pytest.mark.parametrize("T,n,mode,prune", VISION, ids=lambda v: str(v))
def test_vision_tower_every_stage(T, n, mode, prune, monkeypatch):
    monkeypatch.setenv("IVR_PRUNE_LAST", str(prune))
    monkeypatch.delenv("IVR_FUSED_QKV", raising=False)
    cfg = vision_cfg(T, mode)
    spec, W, caps, prev, out, x = capture_run(cfg, mode, n)
    res = S.check_tower(spec, W, caps, n=n, T=T, pruned_last=bool(prune), out=out, normalize=True, patches=x, prev_caps=prev)
    kinds = {r[0] for r in res}
    assert {"embed", "ln1", "qkv", "attention", "attn_out", "ln2", "pool_ln", "f_normalize"} <= kinds, kinds
    assert ("fc1_cls" in kinds) == bool(prune or spec.cls_bf16) and ("hid8" in kinds or "hid_cls8" in kinds) == (mode == "fp8_all_fc2")
    check(res, f"T={T} n={n} {mode} prune={prune}:")


def text_ids(T):
    """first EOS at 0, at T-1, in the middle with more behind it, absent; an id below 0 and one >= vocab"""
    rng = np.random.default_rng(T)
    ids = rng.integers(1, TEXT.vocab - 1, (6, T))
    ids[0, 0] = TEXT.eos_id
    ids[1, T - 1] = TEXT.eos_id
    ids[2, T // 2] = ids[2, T // 2 + 3] = ids[2, T - 1] = TEXT.eos_id
    ids[4, 1], ids[4, T // 3] = -5, TEXT.eos_id
    ids[5, 2], ids[5, T - 2] = TEXT.vocab + 7, TEXT.eos_id
    return torch.from_numpy(ids.astype(np.int64))


@pytest.mark.parametrize("T", [77, 20])
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_text_tower_every_stage(T, mode):
    ids = text_ids(T)
    n = ids.shape[0]
    prev_ids = torch.from_numpy(np.random.default_rng(1).integers(0, TEXT.vocab, (2 * n + 3, T)))
    spec, W, caps, prev, out, x = capture_run(TEXT, mode, n, ids=ids, prev_ids=prev_ids)
    assert caps[(0, "eos_pos")][:n, 0].tolist() == [0, T - 1, T // 2, 0, T // 3, T - 2]
    res = S.check_tower(spec, W, caps, n=n, T=T, pruned_last=False, out=out, normalize=True, ids=x, prev_caps=prev)
    assert {"embed", "eos_pos", "pool_ln", "proj", "f_normalize"} <= {r[0] for r in res}
    check(res, f"text T={T} {mode}:")


def zero_post_ln(w):
    w["post_ln_g"][:] = 0
    w["post_ln_b"][:] = 0


def tiny_post_ln(w):
    w["post_ln_g"] *= np.float32(1e-14)
    w["post_ln_b"] *= np.float32(1e-14)


@pytest.mark.parametrize("case", ["zero", "tiny", "raw"])
def test_f_normalize_edge_rows(case, monkeypatch):
    """f_normalize has no entry point of its own, so its edge rows are reached by weights: post-LN gain and bias 0 pool a zero row
    (0 / 1e-12 = 0 exactly), scaled by 1e-14 a row of norm below 1e-12 (divided by 1e-12f); normalize = 0 copies to the bit."""
    monkeypatch.delenv("IVR_FUSED_QKV", raising=False)
    monkeypatch.delenv("IVR_PRUNE_LAST", raising=False)
    cfg = vision_cfg(10, "bf16")
    wmod = {"zero": zero_post_ln, "tiny": tiny_post_ln, "raw": None}[case]
    spec, W, caps, prev, out, x = capture_run(cfg, "bf16", 5, normalize=case != "raw", wmod=wmod)
    pooled = caps[(0, "pooled")][:5].double()
    if case == "zero":
        assert not pooled.any() and not out.any()
    if case == "tiny":
        assert 0 < float(pooled.norm(dim=1).max()) < 1e-12
    res = S.check_tower(spec, W, caps, n=5, T=10, pruned_last=True, out=out, normalize=case != "raw", patches=x, prev_caps=prev)
    check(res, f"f_normalize {case}:")


# ---- the same bits on every path ---------------------------------------------------------------------------------------------------
def _caps(cfg, mode, n, env, monkeypatch):
    for k in ("IVR_FUSED_QKV", "IVR_QKV_PERS", "IVR_ZIGZAG", "IVR_PRUNE_LAST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    spec, _, caps, _, out, _ = capture_run(cfg, mode, n)
    return spec, caps, out


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(S.raw(a), S.raw(b))


def _compare_all(spec, a, b, n, T, pruned, skip=()):
    """every site both runs materialised, bit for bit (a pruned last block under the fused kernel holds query 0 in att[0, n))"""
    L, diff = spec.cfg.layers, []
    for key in S.capture_list(spec):
        x, y = a.get(key), b.get(key)
        if key[1] in skip or x is None or y is None:
            continue
        if key == (L - 1, "att") and pruned:
            x, y = (x[:n] if a.get((L - 1, "qkv")) is None else x[0::T]), (y[:n] if b.get((L - 1, "qkv")) is None else y[0::T])
        if not _same_bits(x.contiguous(), y.contiguous()):
            diff.append(key)
    return diff


@pytest.mark.parametrize("T,n,mode,prune", [(10, 23, "bf16", "1"), (50, 5, "bf16", "0"), (50, 5, "fp8_all_o", "1"), (10, 23, "fp8_mlp", "1"),
                                            (50, 1, "bf16", "1")], ids=lambda v: str(v))
def test_fused_qkv_attention_same_bits_at_every_site(T, n, mode, prune, monkeypatch):
    cfg = vision_cfg(T, mode)
    spec, ref, out_ref = _caps(cfg, mode, n, {"IVR_FUSED_QKV": "0", "IVR_PRUNE_LAST": prune}, monkeypatch)
    assert ref[(0, "qkv")] is not None
    for pers in ("0", "2"):
        _, got, out = _caps(cfg, mode, n, {"IVR_FUSED_QKV": "1", "IVR_QKV_PERS": pers, "IVR_PRUNE_LAST": prune}, monkeypatch)
        assert all(got[(i, "qkv")] is None for i in range(cfg.layers)), "the fused kernel did not run"
        assert _compare_all(spec, got, ref, n, T, prune == "1") == [] and torch.equal(out, out_ref)


@pytest.mark.parametrize("T,n,mode", [(65, 5, "bf16"), (50, 23, "fp8_mlp"), (10, 5, "f32")], ids=lambda v: str(v))
def test_zigzag_same_bits_at_every_site(T, n, mode, monkeypatch):
    cfg = vision_cfg(T, mode)
    spec, a, out_a = _caps(cfg, mode, n, {"IVR_ZIGZAG": "0"}, monkeypatch)
    _, b, out_b = _caps(cfg, mode, n, {"IVR_ZIGZAG": "1"}, monkeypatch)
    assert _compare_all(spec, a, b, n, T, False) == [] and torch.equal(out_a, out_b)


@pytest.mark.parametrize("T,n,mode", [(50, 5, "bf16"), (10, 23, "fp8_mlp"), (65, 5, "fp8_all_fc2"), (10, 5, "f32")], ids=lambda v: str(v))
def test_pruned_last_block_same_bits_on_the_rows_both_write(T, n, mode, monkeypatch):
    cfg = vision_cfg(T, mode)
    L = cfg.layers
    spec, full, out_f = _caps(cfg, mode, n, {"IVR_PRUNE_LAST": "0"}, monkeypatch)
    _, pr, out_p = _caps(cfg, mode, n, {"IVR_PRUNE_LAST": "1"}, monkeypatch)
    # everything in front of the last block's attn-out is the same launch sequence
    head = [k for k in S.capture_list(spec) if k[1] not in ("pool_ln", "pooled") and (k[0] < L - 1 or (k[0] == L - 1 and k[1] in ("stream", "ln1", "qkv", "att")))]
    assert _compare_all(spec, {k: pr.get(k) for k in head}, {k: full.get(k) for k in head}, n, T, False) == []
    side = spec.side(L - 1)
    pairs = [(pr[(L - 1, "attn_out")][0::T], full[(L - 1, "attn_out")][0::T]),
             (pr[(L - 1, "ln2")][:n], full[(L - 1, "ln2_cls")][:n] if side else full[(L - 1, "ln2")][0::T]),
             (pr[(L - 1, "hid_cls")][:n], full[(L - 1, "hid_cls")][:n] if side else full[(L - 1, "hid")][0::T]),
             (pr[(L, "stream")][0::T], full[(L, "stream")][0::T]),
             (pr[(0, "pool_ln")][:n], full[(0, "pool_ln")][:n]), (pr[(0, "pooled")][:n], full[(0, "pooled")][:n]), (out_p, out_f)]
    if mode == "fp8_all_fc2":
        pairs.append((pr[(L - 1, "hid_cls8")][:n], full[(L - 1, "hid8")][0::T]))
    assert [i for i, (x, y) in enumerate(pairs) if not _same_bits(x.contiguous(), y.contiguous())] == []
    # and the pruned block leaves every other row of the stream as it found it
    rest = torch.ones(n * T, dtype=torch.bool)
    rest[0::T] = False
    assert torch.equal(pr[(L, "stream")][rest.cuda()], pr[(L - 1, "stream")][rest.cuda()])
