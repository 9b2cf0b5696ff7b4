"""GPU suite of ivr_amd/keyframes.py (csrc/phash.hip, csrc/keepwin.hip): the hash kernel for exact equality with Pillow (the 32x32
image) and with phash_ref (the 8 bytes), the two look-back filters for exact equality with their numpy definitions, ivr_resize_u8
against Pillow, and select_keyframes against its composition in numpy."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import keyframe_cases as K
from ivr_amd import keyframes
from ivr_amd.preprocess import resize_frames_u8
from oracle.reduce_ref import flat_score_bound

pytestmark = pytest.mark.gpu

WINDOWS = (1, 10, 64)


# -- the hash ------------------------------------------------------------------------------------------------------------------
def constant_frames(seed, n, h, w):
    return np.stack([np.full((h, w, 3), v, np.uint8) for v in (77, 0, 255)][:n])


@pytest.mark.parametrize("n,h,w,bgr,maker", [
    (1, 32, 32, False, K.mixed_frames),            # both passes skipped
    (3, 224, 224, False, K.mixed_frames),          # the reference's own shape
    (2, 33, 47, False, K.mixed_frames),            # w * 3 unaligned, barely any downscale
    (2, 17, 500, False, K.mixed_frames),           # upscale on one axis, strong downscale on the other
    (1, 31, 31, False, K.mixed_frames),            # upscale on both axes
    (2, 1, 1, False, K.noise_frames),
    (1, 1080, 1920, False, K.mixed_frames),        # many bands, 363 taps
    (70, 64, 48, False, K.mixed_frames),           # frame indexing past one wave of frames
    (5, 224, 224, True, K.mixed_frames),
    (3, 40, 56, False, constant_frames),           # the coefficients are rounding residue: the kernel's must be the definition's
    (2, 32, 500, False, K.mixed_frames),           # only the vertical pass skipped
    (2, 500, 32, True, K.mixed_frames),            # only the horizontal pass skipped
])
def test_hash_and_pixels_are_exact(n, h, w, bgr, maker):
    frames = maker(11, n, h, w)
    want_hash, want_px = keyframes.phash_ref(frames, bgr=bgr, return_pixels=True)
    for i, f in enumerate(frames):
        assert np.array_equal(want_px[i], K.pillow_pixels(f[..., ::-1] if bgr else f))       # Pillow itself, from the RGB frame
    got_hash, got_px = keyframes.phash(frames, bgr=bgr, return_pixels=True)
    assert got_px.dtype == np.uint8 and got_px.shape == (n, 32, 32) and got_hash.dtype == np.uint8 and got_hash.shape == (n, 8)
    assert np.array_equal(got_px, want_px), f"pixels differ in frames {np.flatnonzero((got_px != want_px).any(axis=(1, 2)))[:10]}"
    assert np.array_equal(got_hash, want_hash), [(g.tobytes().hex(), w_.tobytes().hex()) for g, w_ in zip(got_hash, want_hash)][:4]
    if n >= 3 and maker is K.mixed_frames:
        assert len({h_.tobytes() for h_ in got_hash}) == n                                   # all frames different, all hashes too
    # without the pixels, and from a tensor that is on the device already
    assert np.array_equal(keyframes.phash_device(torch.from_numpy(frames).cuda(), bgr=bgr).cpu().numpy(), want_hash)


def test_unaligned_frame_buffers_and_other_streams():
    """A batch that starts 1, 2, 3 and 5 bytes into its allocation (the 16-byte loads of the row kernel have a ragged head and tail
    in every band), and one run on a stream of its own."""
    frames = K.mixed_frames(5, 3, 45, 51)
    want = keyframes.phash_ref(frames, return_pixels=True)
    for shift in (1, 2, 3, 5):
        buf = torch.zeros(frames.size + 64, dtype=torch.uint8, device="cuda")
        view = buf[shift:shift + frames.size].view(frames.shape)
        view.copy_(torch.from_numpy(frames))
        got = keyframes.phash_device(view, return_pixels=True)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = keyframes.phash_device(frames)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), want[0])


def test_no_frames():
    h, p = keyframes.phash(np.zeros((0, 24, 24, 3), np.uint8), return_pixels=True)
    assert h.shape == (0, 8) and p.shape == (0, 32, 32)
    assert keyframes.hash_keep_mask(np.zeros((0, 8), np.uint8)).shape == (0,)
    assert keyframes.kept_window_mask(np.zeros((0, 16), np.float32)).shape == (0,)
    assert [len(a) for a in keyframes.select_keyframes(np.zeros((0, 16), np.float32), np.zeros((0, 8), np.uint8))] == [0, 0]


@pytest.mark.parametrize("mode,bilinear,h,w", [("stretch", False, 72, 96), ("stretch", False, 300, 131), ("stretch", True, 300, 131),
                                               ("letterbox", False, 72, 96), ("letterbox", False, 300, 131),
                                               ("shortest_edge_crop", False, 250, 330), ("shortest_edge_crop", False, 300, 231)])
def test_resize_frames_u8_is_pillow(mode, bilinear, h, w):
    frames = K.mixed_frames(3, 3, h, w)
    got = resize_frames_u8(frames, mode, 224, bilinear)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 224, 224, 3) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), K.pillow_resize(frames, 224, mode, bilinear))


def test_resize_of_a_frame_that_has_the_size_already_is_a_copy():
    frames = K.noise_frames(1, 2, 224, 224)
    for mode in ("identity", "stretch"):
        assert np.array_equal(resize_frames_u8(frames, mode, 224).cpu().numpy(), frames)
    # the reference's route: stretch to 224 x 224 (:246), then hash what the embedder sees
    big = K.mixed_frames(2, 2, 360, 640)
    small = resize_frames_u8(big[..., ::-1].copy(), "stretch", 224)                             # BGR in, BGR out
    assert np.array_equal(keyframes.phash_device(small, bgr=True).cpu().numpy(), keyframes.phash_ref(K.pillow_resize(big, 224, "stretch")))


# -- the two filters -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hashes():
    return K.hash_walk(K.N_ROWS, 1)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("threshold", [0, 5, 64])
def test_hash_keep_mask_is_its_definition(threshold, window):
    h = hashes()
    for seg in (None, K.SEGMENTS, torch.from_numpy(K.SEGMENTS).cuda()):
        want = keyframes.hash_keep_mask_ref(h, None if seg is None else K.SEGMENTS, threshold, window)
        got = keyframes.hash_keep_mask(h, seg, threshold, window)
        assert got.dtype == np.uint8 and np.array_equal(got, want), f"rows {np.flatnonzero(got != want)[:10]}"
    inside = want[K.SEGMENTS[0]:K.SEGMENTS[-1]]
    assert not want[:K.SEGMENTS[0]].any() and not want[K.SEGMENTS[-1]:].any()
    if threshold == 5:
        assert 0.2 * len(inside) < inside.sum() < 0.9 * len(inside)       # some rows are dropped, not all
        if window > 1:                                                    # and the size of the window decides
            assert inside.sum() < keyframes.hash_keep_mask_ref(h, K.SEGMENTS, 5, 1).sum() - 50


def test_many_short_segments_run_side_by_side():
    h = K.hash_walk(3000, 9)
    off = np.sort(np.random.default_rng(3).integers(0, 3001, 400)).astype(np.int64)
    assert np.array_equal(keyframes.hash_keep_mask(h, off), keyframes.hash_keep_mask_ref(h, off))
    e = K.embedding_walk(900, 100, 9)
    off = np.sort(np.random.default_rng(4).integers(0, 901, 130)).astype(np.int64)
    assert np.array_equal(keyframes.kept_window_mask(e, off), keyframes.kept_window_mask_ref(e, off))


@functools.lru_cache(maxsize=None)
def window_case(d, window):
    """(emb, the definition's mask, the float64 loop's mask and margin) over SEGMENTS: computed once, left unchanged."""
    emb = K.embedding_walk(K.N_ROWS, d, 8)
    want64, margin = K.reference_window_filter(emb, K.SEGMENTS, 0.95, window)
    return emb, keyframes.kept_window_mask_ref(emb, K.SEGMENTS, 0.95, window), want64, margin


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("d", [48, 100, 384, 512])
def test_kept_window_mask_is_its_definition(d, window):
    emb, want, want64, margin = window_case(d, window)
    got = keyframes.kept_window_mask(emb, K.SEGMENTS, 0.95, window)
    assert got.dtype == np.uint8 and np.array_equal(got, want), f"rows {np.flatnonzero(got != want)[:10]}"       # no margin: the arithmetic is reproduced
    assert margin > 1e-5, f"seed puts a float64 cosine within 1e-5 of the threshold ({margin:.2e})"
    assert np.array_equal(got, want64)
    inside = got[K.SEGMENTS[0]:K.SEGMENTS[-1]]
    assert not got[:K.SEGMENTS[0]].any() and not got[K.SEGMENTS[-1]:].any() and got[3] == 1 and got[20] == 1
    assert 0.1 * len(inside) < inside.sum() < 0.9 * len(inside)
    if window > 1:                                 # the size of the window decides: a smaller one keeps more rows
        assert inside.sum() < window_case(d, 1)[1].sum() - 50
    if window == 10:
        dev = torch.from_numpy(emb).cuda()
        assert np.array_equal(keyframes.kept_window_mask_device(dev, torch.from_numpy(K.SEGMENTS).cuda(), 0.95, window).cpu().numpy(), want)
        assert np.array_equal(keyframes.kept_window_mask(emb[:300], None, 0.95, window), keyframes.kept_window_mask_ref(emb[:300], None, 0.95, window))


def test_zero_rows_and_a_window_that_reaches_far_back():
    e = np.zeros((45, 8), np.float32)
    e[:42, 0], e[42, 1] = 1, 1                     # rows 43, 44 are zero: cosine 0 to everything (a zero norm counts as 1)
    assert keyframes.kept_window_mask(e, None, 0.95, 1).tolist() == [1] + [0] * 41 + [1, 1, 1]
    assert keyframes.kept_window_mask(e, None, 0.0, 2).tolist() == [1] + [0] * 44
    h = np.zeros((43, 8), np.uint8)
    h[42] = 255
    assert keyframes.hash_keep_mask(h, None, 5, 1).tolist() == [1] + [0] * 41 + [1]


# -- phases 2-4 and the class --------------------------------------------------------------------------------------------------
def test_select_keyframes_is_its_composition_in_numpy():
    d, video_off = 384, np.array([0, 170, 170, 300], np.int64)
    emb, h = K.video_embeddings([170, 0, 130], d, 3), K.hash_walk(300, 4)
    _, _, m = K.reference_select_keyframes(emb, h, video_off)
    assert m["eps"] > flat_score_bound(d, 1.0), m          # the one step whose float32 scores numpy does not reproduce bit for bit
    want_rows, want_scenes = keyframes.select_keyframes_ref(emb, h, video_off)
    rows, scenes = keyframes.select_keyframes(emb, h, video_off)
    assert rows.dtype == np.int64 and np.array_equal(rows, want_rows) and np.array_equal(scenes, want_scenes)
    assert 20 < len(rows) < 200 and (rows >= 170).any() and (rows < 170).any()
    rows_dev, _ = keyframes.select_keyframes(torch.from_numpy(emb).cuda(), torch.from_numpy(h).cuda(), video_off)
    assert np.array_equal(rows_dev, want_rows)
    one, _ = keyframes.select_keyframes(emb[:170], h[:170])
    assert np.array_equal(one, want_rows[want_rows < 170])


def test_extractor_methods_agree_with_the_kernels():
    ex = keyframes.AdvancedKeyframeExtractor()
    h = hashes()[:400]
    values = [keyframes.PerceptualHash(x) for x in h]
    keep, window = [], []
    for v in values:                               # filter_research_update.py:293-298 with the class's own method
        if not ex.is_duplicate_by_hash(v, window):
            keep.append(1)
            window.append(v)
            if len(window) > keyframes.TEMPORAL_WINDOW:
                window.pop(0)
        else:
            keep.append(0)
    assert keyframes.hash_keep_mask(h).tolist() == keep and 0 < sum(keep) < 400
    frame = K.sinusoid_frames(4, 1, 224, 224)[0]
    value = ex.extract_perceptual_hash(frame)
    assert str(value) == K.imagehash_phash(frame)[0].tobytes().hex() and value - value == 0
    assert ex.extract_perceptual_hash(Image.fromarray(frame)) == value
    emb = K.video_embeddings([60], 48, 8)
    cuts = ex.detect_scene_changes(list(emb))
    e64 = emb.astype(np.float64)
    sims = np.sum(e64[1:] * e64[:-1], axis=1) / (np.linalg.norm(e64[1:], axis=1) * np.linalg.norm(e64[:-1], axis=1))
    assert np.abs(sims - 0.7).min() > 1e-5 and cuts == [0] + (1 + np.flatnonzero(sims < 0.7)).tolist() + [60] and len(cuts) > 2


def test_extract_advanced_keyframes_is_resize_hash_embed_select():
    """The class's driver against its own steps done by hand: Pillow's stretch to 224 x 224 of the RGB frame, the hash of that image,
    the random-init DINO tower in float32 on it, select_keyframes."""
    from ivr_amd.compat import FrameFilter
    rgb = np.concatenate([K.sinusoid_frames(s, 1, 90, 120) for s in (1, 1, 1, 2, 2, 3, 3, 3, 3, 4)])
    rgb[1:3] = np.minimum(rgb[1:3].astype(np.int32) + 1, 255)       # near copies: the same hash, or all but
    ff = FrameFilter(allow_random_init=True, compute="f32", max_batch=4)
    ex = keyframes.AdvancedKeyframeExtractor(ff)
    pts = [i / 25 for i in range(len(rgb))]
    got = ex.extract_advanced_keyframes(np.ascontiguousarray(rgb[..., ::-1]), pts)
    small = K.pillow_resize(rgb, 224, "stretch")
    emb = ff.tower.encode_frames(small, "identity", ff.mean, ff.std, normalize=False)
    rows, scenes = keyframes.select_keyframes(emb, keyframes.phash_ref(small))
    assert [g["original_frame_idx"] for g in got] == rows.tolist() and [g["scene_id"] for g in got] == scenes.tolist()
    assert [g["n"] for g in got] == list(range(len(rows))) and [g["pts_time"] for g in got] == [round(pts[r], 3) for r in rows]
    assert 1 <= len(rows) <= len(rgb)              # which frames survive is the random-init tower's affair: select_keyframes has its own test
    assert np.allclose(ex.extract_embedding(Image.fromarray(small[0])), emb[0].cpu().numpy(), rtol=0, atol=1e-3 * float(emb[0].abs().max()))
