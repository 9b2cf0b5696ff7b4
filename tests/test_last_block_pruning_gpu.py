"""GPU parity of the pruned last block (IVR_PRUNE_LAST, default on): the vision towers pool row i*T (token 0) of the final residual
stream only, so the last block runs attention output, attn-out, LN2, fc1 and fc2 on those n rows alone.  Every launch on those rows
does the same arithmetic in the same order as the full block (a GEMM row does not depend on M or on the kernel the size picks, the
pooled mode of the fused QKV + attention kernel runs the very unit that held query 0), so the embeddings must be BIT-identical to
IVR_PRUNE_LAST=0: np.array_equal, no tolerance."""
import numpy as np
import pytest
import torch

from conftest import synth_frames
from ivr_amd import config as C
from ivr_amd.weights import make_weights

pytestmark = pytest.mark.gpu


def _encode(cfg, w, frames, monkeypatch, prune, env=(), **kw):
    from ivr_amd.tower import Tower
    for k, v in env:
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("IVR_PRUNE_LAST", "1" if prune else "0")
    mean, std = (C.IMAGENET_MEAN, C.IMAGENET_STD) if cfg is C.DINO_VIT_S16 else (C.CLIP_MEAN, C.CLIP_STD)
    tw = Tower(cfg, w, max_batch=len(frames), **kw)
    out = tw.encode_frames(frames, "identity", mean, std).cpu().numpy()
    del tw
    return out


def _same(cfg, w, frames, monkeypatch, env=(), **kw):
    a = _encode(cfg, w, frames, monkeypatch, True, env, **kw)
    b = _encode(cfg, w, frames, monkeypatch, False, env, **kw)
    assert np.isfinite(b).all()
    assert np.array_equal(a, b), np.abs(a - b).max()
    return a


@pytest.mark.parametrize("fused,pers", [("1", "0"), ("1", "2"), ("0", "0")], ids=lambda v: str(v))
@pytest.mark.parametrize("n", [1, 5, 23])
def test_vit_b32_bf16_small_batches(n, fused, pers, monkeypatch):
    cfg = C.CLIP_VIT_B32
    w = make_weights(cfg, 12)
    _same(cfg, w, synth_frames(700 + n, n, 224, 224), monkeypatch, (("IVR_FUSED_QKV", fused), ("IVR_QKV_PERS", pers)))


@pytest.mark.parametrize("fused,pers", [("1", "0"), ("1", "2"), ("0", "0")], ids=lambda v: str(v))
def test_vit_b32_bf16_large_batch(fused, pers, monkeypatch):
    """640 images: the 256 x 256 GEMMs (and their persistent form) on the full rows, the skinny / 128 x 128 kernels would be picked
    for none of the pruned launches either (640 rows), so both sides differ in every GEMM's kernel choice."""
    cfg = C.CLIP_VIT_B32
    w = make_weights(cfg, 12)
    _same(cfg, w, synth_frames(31, 640, 224, 224), monkeypatch, (("IVR_FUSED_QKV", fused), ("IVR_QKV_PERS", pers)))


def test_vit_b32_f32(monkeypatch):
    cfg = C.CLIP_VIT_B32
    _same(cfg, make_weights(cfg, 12), synth_frames(41, 7, 224, 224), monkeypatch, compute="f32")


@pytest.mark.parametrize("compute,sites", [("fp8", None), ("fp8_mlp", None), ("fp8_all", None), ("fp8_all", ("o",)),
                                           ("fp8_all", ("fc2",))], ids=lambda v: str(v))
@pytest.mark.parametrize("n", [5, 300])
def test_vit_b32_fp8_presets(compute, sites, n, monkeypatch):
    """fp8 / fp8_mlp: the token-0 rows take the bf16 side path (the pruned block launches no e4m3 MLP GEMM); fp8_all: e4m3 attn-out,
    LN2 -> e4m3, fc1 writing e4m3, fc2 on n rows; fc2 alone in e4m3: the bf16 -> e4m3 copy of the hidden rows."""
    cfg = C.CLIP_VIT_B32
    kw = {"compute": compute} if sites is None else {"compute": compute, "fp8_sites": sites}
    _same(cfg, make_weights(cfg, 12), synth_frames(51 + n, n, 224, 224), monkeypatch, (("IVR_FUSED_QKV", "1"),), **kw)


def test_dino_vit_s16(monkeypatch):
    """T = 197: unfused attention, LN_ALL_CLS pooling."""
    cfg = C.DINO_VIT_S16
    _same(cfg, make_weights(cfg, 3), synth_frames(61, 6, 224, 224), monkeypatch)


def test_tiny_vit(monkeypatch):
    cfg = C.TINY_VIT
    _same(cfg, make_weights(cfg, 5), synth_frames(71, 9, 224, 224), monkeypatch)


def test_capture_of_the_final_residual_runs_the_full_block(monkeypatch):
    """A debug capture of layer `layers` reads every row of the final residual stream: that call runs the last block in full."""
    from ivr_amd.preprocess import preprocess_frames
    from ivr_amd.tower import Tower
    cfg = C.CLIP_VIT_B32
    w = make_weights(cfg, 12)
    frames = synth_frames(81, 5, 224, 224)
    px = preprocess_frames(frames, "identity", patch=cfg.patch, out_dtype=torch.bfloat16)
    hid = {}
    for prune in ("1", "0"):
        monkeypatch.setenv("IVR_PRUNE_LAST", prune)
        tw = Tower(cfg, w, max_batch=5)
        emb, h = tw.encode_patches(px, 5, capture_hidden=cfg.layers)
        hid[prune] = (emb.cpu().numpy(), h.cpu().numpy())
        del tw
    assert np.array_equal(hid["1"][1], hid["0"][1])
    assert np.array_equal(hid["1"][0], hid["0"][0])
    # the next call (no capture) is pruned again and still yields the same embedding
    monkeypatch.setenv("IVR_PRUNE_LAST", "1")
    tw = Tower(cfg, w, max_batch=5)
    tw.encode_patches(px, 5, capture_hidden=cfg.layers)
    assert np.array_equal(tw.encode_patches(px, 5).cpu().numpy(), hid["0"][0])
