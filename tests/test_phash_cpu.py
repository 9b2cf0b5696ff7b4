"""CPU suite of ivr_amd/keyframes.py (csrc/phash.hip, csrc/keepwin.hip): the numpy + Pillow definitions against the reference's code
restated around Pillow, scipy and sklearn (tests/keyframe_cases.py; imagehash itself is not installed), the cosine table of the
library, the ABI of the new entry points and the checks that need no device.  No compute call reaches a device."""
import ctypes
import re

import numpy as np
import pytest

import keyframe_cases as K
from conftest import ROOT
from ivr_amd import _ffi, keyframes
from ivr_amd.binary import BinaryFlatIndex
from ivr_amd.index import FlatIPIndex
from oracle.reduce_ref import flat_score_bound

NEW = {
    "ivr_resize_u8": ["ctx", "src", "n", "h", "w", "flags", "out_size", "dst", "stream"],
    "ivr_phash": ["ctx", "src", "n", "h", "w", "flags", "hash", "pixels", "stream"],
    "ivr_hash_keep_mask": ["ctx", "hashes", "n", "seg_off", "nseg", "threshold", "window", "keep", "stream"],
    "ivr_kept_window_mask": ["ctx", "emb", "n", "d", "seg_off", "nseg", "threshold", "window", "keep", "stream"],
}
SIZES = ((224, 224), (33, 47), (1080, 1920), (32, 32), (17, 500))


# -- the hash ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("family", sorted(K.FAMILIES))
def test_phash_ref_is_imagehash_restated(family, h, w):
    """Bit for bit, no exempt bits.  Direct summation and scipy's FFT differ by some 1e-10 at most, so the inputs must keep every
    coefficient further than 1e-6 from its median: a condition on the inputs, asserted first."""
    frames = K.FAMILIES[family](7, 2 if h * w > 10 ** 6 else 4, h, w)
    hashes, pixels = keyframes.phash_ref(frames, return_pixels=True)
    assert hashes.shape == (len(frames), 8) and hashes.dtype == np.uint8 and pixels.shape == (len(frames), 32, 32)
    for f, got, px in zip(frames, hashes, pixels):
        want, low, med = K.imagehash_phash(f)
        assert np.abs(low - med).min() > 1e-6, f"seed puts a coefficient within 1e-6 of the median ({np.abs(low - med).min():.2e})"
        assert np.array_equal(px, K.pillow_pixels(f))
        assert np.array_equal(got, want), f"{got.tobytes().hex()} != {want.tobytes().hex()}"
    assert len({h_.tobytes() for h_ in hashes}) > 1
    # BGR input is the same frames with the channels swapped
    assert np.array_equal(keyframes.phash_ref(np.ascontiguousarray(frames[..., ::-1]), bgr=True), hashes)


def test_constant_frame_follows_the_definition():
    """The one departure: on a constant frame every coefficient but B[0][0] is rounding residue, here of the direct sums, in the
    reference of its FFT, so those 63 bits are not compared with the reference (the GPU suite holds the kernel to phash_ref there).
    What the definition fixes: B[0][0] = 4 * 1024 * grey is the largest value, and a black frame has no bit set."""
    frames = np.full((3, 40, 56, 3), 77, np.uint8)
    frames[1] = 0
    frames[2] = 255
    hashes = keyframes.phash_ref(frames)
    assert hashes[0, 0] & 0x80 and hashes[2, 0] & 0x80 and hashes[1].tobytes().hex() == "0000000000000000"
    for f in frames[[0, 2]]:
        low = K.imagehash_phash(f)[1]
        assert abs(low[0, 0] - 4096.0 * f[0, 0, 0]) < 1e-6 and np.abs(low.ravel()[1:]).max() < 1e-9      # the reference's other 63: residue too


def test_cosine_table_is_within_one_ulp_of_numpy():
    C = keyframes.cos_table()
    k, m = np.mgrid[0:8, 0:32]
    want = np.cos(np.pi * (k * (2 * m + 1)).astype(np.float64) / 64.0)
    assert C.shape == (8, 32) and C.dtype == np.float64
    assert (np.abs(C - want) <= np.spacing(np.abs(want))).all()
    assert (C[0] == 1.0).all()


def test_perceptual_hash_value_behaves_like_imagehash():
    a, b = keyframes.PerceptualHash([0xF0, 0, 0, 0, 0, 0, 0, 1]), keyframes.PerceptualHash(np.array([0x0F, 0, 0, 0, 0, 0, 0, 0], np.uint8))
    assert str(a) == "f000000000000001" and a - b == 9 and b - a == 9 and a - a == 0 and a == keyframes.PerceptualHash(a.bytes) and a != b
    ex = keyframes.AdvancedKeyframeExtractor()
    assert ex.is_duplicate_by_hash(a, [b, keyframes.PerceptualHash([0xF0, 0, 0, 0, 0, 0, 0, 0x1F])]) and not ex.is_duplicate_by_hash(a, [b])
    assert not ex.is_duplicate_by_hash(a, [])


# -- the two filters -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 10, 64])
@pytest.mark.parametrize("threshold", [0, 5, 64])
def test_hash_keep_mask_ref_is_the_reference_loop(threshold, window):
    hashes = K.hash_walk(K.N_ROWS, 1)
    for seg in (None, K.SEGMENTS):
        got = keyframes.hash_keep_mask_ref(hashes, seg, threshold, window)
        assert got.dtype == np.uint8 and np.array_equal(got, K.reference_hash_filter(hashes, seg, threshold, window))
    inside = got[K.SEGMENTS[0]:K.SEGMENTS[-1]]
    assert not got[:K.SEGMENTS[0]].any() and not got[K.SEGMENTS[-1]:].any() and got[3] == 1 and got[20] == 1
    if threshold == 5:
        assert 0.2 * len(inside) < inside.sum() < 0.9 * len(inside)       # some rows are dropped, not all
        if window > 1:                                                    # and the size of the window decides
            assert inside.sum() < keyframes.hash_keep_mask_ref(hashes, K.SEGMENTS, 5, 1).sum() - 50
    if threshold == 64:
        assert inside.sum() == 5                                          # the first row of every non-empty segment


@pytest.mark.parametrize("window", [1, 10, 64])
@pytest.mark.parametrize("d", [48, 384])
def test_kept_window_mask_ref_is_the_reference_loop(d, window):
    emb = K.embedding_walk(400, d, 2)
    seg = np.array([2, 2, 3, 30, 31, 380], np.int64)
    for s in (None, seg):
        want, margin = K.reference_window_filter(emb, s, 0.95, window)
        assert margin > 1e-5, f"seed puts a float64 cosine within 1e-5 of the threshold ({margin:.2e})"
        got = keyframes.kept_window_mask_ref(emb, s, 0.95, window)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert not got[:2].any() and not got[380:].any() and got[2] == 1 and got[30] == 1
    assert 0.1 * 378 < got.sum() < 0.9 * 378              # some rows are dropped, not all
    if window > 1:                                        # and the size of the window decides
        assert got.sum() < keyframes.kept_window_mask_ref(emb, seg, 0.95, 1).sum() - 20


def test_the_window_holds_kept_rows_only_and_reaches_far_back():
    """Row 0 is kept, rows 1..40 are its duplicates and dropped, row 41 still meets row 0 in a window of one."""
    h = np.zeros((43, 8), np.uint8)
    h[42] = 255
    assert keyframes.hash_keep_mask_ref(h, None, 5, 1).tolist() == [1] + [0] * 41 + [1]
    e = np.zeros((43, 8), np.float32)
    e[:42, 0], e[42, 1] = 1, 1
    assert keyframes.kept_window_mask_ref(e, None, 0.95, 1).tolist() == [1] + [0] * 41 + [1]
    # the oldest kept row leaves: with a window of one, row 2 equals row 0 but only row 1 is in the window
    e = np.eye(3, dtype=np.float32)[[0, 1, 0]]
    assert keyframes.kept_window_mask_ref(e, None, 0.95, 1).tolist() == [1, 1, 1]
    assert keyframes.kept_window_mask_ref(e, None, 0.95, 2).tolist() == [1, 1, 0]


# -- phases 2-4 ----------------------------------------------------------------------------------------------------------------
def test_select_keyframes_ref_is_the_reference_pipeline():
    d, video_off = 384, np.array([0, 170, 170, 300], np.int64)
    emb, hashes = K.video_embeddings([170, 0, 130], d, 3), K.hash_walk(300, 4)
    rows, scenes, m = K.reference_select_keyframes(emb, hashes, video_off)
    bound = float(flat_score_bound(d, 1.0))
    assert m["scene"] > 1e-5 and m["final"] > 1e-5 and m["eps"] > bound and m["winner"] > bound, m
    got_rows, got_scenes = keyframes.select_keyframes_ref(emb, hashes, video_off)
    assert got_rows.dtype == np.int64 and np.array_equal(got_rows, rows) and np.array_equal(got_scenes, scenes)
    assert 20 < len(rows) < 200 and scenes.max() >= 3 and (rows >= 170).any() and scenes[rows >= 170].min() == 0
    one_rows, _ = keyframes.select_keyframes_ref(emb[:170], hashes[:170])
    assert np.array_equal(one_rows, rows[rows < 170])                # a video does not depend on its neighbours


# -- ABI and surfaces ----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/ivr_api.h").read(), flags=re.S)


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl or decl.startswith("ivr_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


@pytest.mark.parametrize("name", sorted(NEW))
def test_header_binding_and_library_agree(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} not declared in ivr_api.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [re.sub(r"[\s*]+", " ", p).split()[-1] for p in params] == NEW[name]
    res, args = _ffi._SIGS[name]
    assert res is ctypes.c_int and args == [_ctype_of(p) for p in params]
    assert _ffi._STREAM[name] == len(params) - 1
    assert name in _ffi.EXPORTS and name not in _ffi._VALUE
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)


def test_every_new_export_is_classified():
    assert "ivr_phash_scratch_bytes" in _ffi._VALUE and "ivr_phash_scratch_bytes" not in _ffi._STREAM
    assert "ivr_phash_cos_table" not in _ffi._VALUE and "ivr_phash_cos_table" not in _ffi._STREAM
    for name in list(NEW) + ["ivr_phash_scratch_bytes", "ivr_phash_cos_table"]:
        assert name in _ffi._SIGS and re.search(r"\b" + name + r"\s*\(", _header())
    assert _ffi.call("ivr_phash_scratch_bytes", 3, 1080, 1920) >= 3 * 1080 * 32
    assert re.search(r"#define\s+IVR_PHASH_MAX_SIDE\s+%d\b" % _ffi.IVR_PHASH_MAX_SIDE, _header()) and _ffi.IVR_PHASH_MAX_SIDE >= 1920
    assert re.search(r"#define\s+IVR_KEEPWIN_MAX_WINDOW\s+%d\b" % _ffi.IVR_KEEPWIN_MAX_WINDOW, _header())


def test_api_version_is_still_11_and_no_class_grew_a_method():
    assert _ffi.API_VERSION == 11 and _ffi.load().ivr_api_version() == 11
    assert re.search(r"#define\s+IVR_API_VERSION\s+11\b", _header())
    for cls in (FlatIPIndex, BinaryFlatIndex):
        assert not [n for n in dir(cls) if "phash" in n.lower() or "keep" in n.lower() or "keyframe" in n.lower()]


def test_library_rejects_bad_arguments_before_any_device_call():
    lib = _ffi.load()
    one = ctypes.c_void_p(1)                   # never dereferenced: every call below fails its checks first

    def rejected(rc, word):
        assert rc == -1 and word.encode() in lib.ivr_last_error(None), lib.ivr_last_error(None)
    rejected(lib.ivr_phash(None, None, 0, 8, 8, 0, None, None, None), "NULL")
    rejected(lib.ivr_phash(one, None, 1, 8, 8, 0, None, None, None), "NULL")
    rejected(lib.ivr_phash(one, one, 1, 8, _ffi.IVR_PHASH_MAX_SIDE + 1, 0, one, None, None), "w=8193")
    rejected(lib.ivr_phash(one, one, 1, 0, 8, 0, one, None, None), "h=0")
    rejected(lib.ivr_phash(one, one, 1, 8, 8, _ffi.PP_OUT_F32, one, None, None), "flags")
    rejected(lib.ivr_phash_cos_table(None), "NULL")
    rejected(lib.ivr_resize_u8(None, None, 0, 8, 8, 2, 224, None, None), "NULL")
    rejected(lib.ivr_resize_u8(one, None, 1, 8, 8, 2, 224, None, None), "NULL")
    rejected(lib.ivr_resize_u8(one, one, 1, 8, 8, 2 | _ffi.PP_BGR, 224, one, None), "flags")
    rejected(lib.ivr_resize_u8(one, one, 1, 8, 8, 2, 100, one, None), "out_size=100")
    rejected(lib.ivr_hash_keep_mask(None, None, 0, None, 0, 5, 10, None, None), "NULL")
    rejected(lib.ivr_hash_keep_mask(one, None, 4, None, 0, 5, 10, None, None), "NULL")
    rejected(lib.ivr_hash_keep_mask(one, one, 4, None, 0, 5, 0, one, None), "window=0")
    rejected(lib.ivr_hash_keep_mask(one, one, 4, None, 0, 5, 65, one, None), "window=65")
    rejected(lib.ivr_hash_keep_mask(one, one, 4, None, 2, 5, 10, one, None), "seg_off")
    rejected(lib.ivr_kept_window_mask(None, None, 0, 4, None, 0, 0.95, 10, None, None), "NULL")
    rejected(lib.ivr_kept_window_mask(one, None, 4, 4, None, 0, 0.95, 10, None, None), "NULL")
    rejected(lib.ivr_kept_window_mask(one, one, 4, 0, None, 0, 0.95, 10, one, None), "d=0")
    rejected(lib.ivr_kept_window_mask(one, one, 4, 4, None, 0, 0.95, 65, one, None), "window=65")
    rejected(lib.ivr_kept_window_mask(one, one, 4, 4, None, 0, float("nan"), 10, one, None), "NaN")


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("phash", "phash_device", "phash_ref", "hash_keep_mask", "hash_keep_mask_device", "hash_keep_mask_ref",
                 "kept_window_mask", "kept_window_mask_device", "kept_window_mask_ref", "select_keyframes", "select_keyframes_ref",
                 "AdvancedKeyframeExtractor", "PerceptualHash"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(keyframes, name)
    assert (keyframes.SIM_THRESHOLD, keyframes.SCENE_THRESHOLD, keyframes.PERCEPTUAL_THRESHOLD, keyframes.TEMPORAL_WINDOW) == (0.95, 0.7, 5, 10)
    from ivr_amd.preprocess import resize_frames_u8  # noqa: F401


def test_argument_checks_name_the_offending_values():
    h, e = np.zeros((4, 8), np.uint8), np.zeros((4, 6), np.float32)
    for fn, x in ((keyframes.hash_keep_mask_ref, h), (keyframes.kept_window_mask_ref, e), (keyframes.hash_keep_mask_device, h),
                  (keyframes.kept_window_mask_device, e)):
        with pytest.raises(ValueError, match=r"window=0 outside \[1,64\]"):
            fn(x, None, 5 if x is h else 0.95, 0)
        with pytest.raises(ValueError, match=r"window=65 outside \[1,64\]"):
            fn(x, None, 5 if x is h else 0.95, 65)
        with pytest.raises(ValueError, match="window must be an integer, got float"):
            fn(x, None, 5 if x is h else 0.95, 2.5)
    with pytest.raises(ValueError, match="threshold must be an integer, got float"):
        keyframes.hash_keep_mask_device(h, None, 5.0)
    with pytest.raises(ValueError, match="not NaN"):
        keyframes.kept_window_mask_device(e, None, float("nan"))
    with pytest.raises(ValueError, match=r"uint8 \[n,h,w,3\]"):
        keyframes.phash_device(np.zeros((2, 8, 8, 3), np.float32))
    with pytest.raises(ValueError, match=r"w=9000 outside \[1,8192\]"):
        keyframes.phash_device(np.zeros((1, 1, 9000, 3), np.uint8))
    with pytest.raises(ValueError, match=r"video_off must ascend from 0 to 4"):
        keyframes.select_keyframes(e, h, np.array([0, 3]))
    with pytest.raises(ValueError, match="3 hashes for 4 embeddings"):
        keyframes.select_keyframes(e, h[:3])
    with pytest.raises(RuntimeError, match="no FrameFilter"):
        keyframes.AdvancedKeyframeExtractor().extract_embedding(None)
