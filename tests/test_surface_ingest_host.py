"""CPU: the host side of the surface ingest: the 10-bit colour rule (tests/surface_ref.py, restated apart from the product)
against the 8-bit rule over the whole lifted cube, against the float64 matrix, and inside int32; SurfaceLayout's defaults,
keys and refusals (simpb_amd/preprocess.py); pack / unpack; the C entry's argument checks, which run before any HIP call.

The three property tests of the rule (lifted cube, float64 closeness, int32 bound) run the WITNESS, surface_ref.convert10, and
no product code: they show that the rule as written down is sound and that the witness may stand for it. The kernel's own
10-bit arithmetic is held to that witness on the GPU (tests/test_gpu_surface_ingest.py, against surface_ref.p010_to_bgr);
of the product, this file checks the coefficients, SurfaceLayout, the plan keys and the C entry's refusals."""
import ctypes

import numpy as np
import pytest

from simpb_amd import preprocess as P
from tests import surface_ref as S
from tests import yuv_ref as Y

STANDARDS10 = ("bt601", "bt709")


# ------------------------------------------------------------------------------------------------------- the 10-bit rule
@pytest.mark.parametrize("standard", STANDARDS10)
def test_coefficients_are_the_eight_bit_ones(standard):
    assert P.p010_coefficients(standard) == P.yuv_coefficients(standard) == Y.integer_matrix(standard)


@pytest.mark.parametrize("standard", STANDARDS10)
def test_lifted_cube_equals_the_eight_bit_rule(standard):
    """An 8-bit sample stored as v << 8 (10-bit value 4 v) gives the 8-bit rule's byte, over the whole 256^3 cube. (Of the
    witness surface_ref.convert10, not of the kernel: see the head of this file.)"""
    cb, cr = np.arange(256)[:, None], np.arange(256)[None, :]
    lift = lambda v: (np.asarray(v).astype(np.int64) << 8) >> 6   # noqa: E731
    for y in range(256):
        want = Y.convert(np.full((1, 1), y), cb, cr, standard)
        got, _ = S.convert10(lift(np.full((1, 1), y)), lift(cb), lift(cr), standard)
        for g, w in zip(got, want):
            assert np.array_equal(np.broadcast_to(g, (256, 256)), np.broadcast_to(w, (256, 256))), (standard, y)


@pytest.mark.parametrize("standard", STANDARDS10)
def test_rule_against_float64_and_inside_int32(standard):
    """All 1024 luma values times a chroma grid (every 16th value and the range ends, centre and extremes: 69 values per
    axis): the integer rule is never more than 1 from the float64 matrix rounded to 8 bits, differs on at most 0.1 % of the
    values (the bound of the 8-bit rule's test; 0.022 % bt601, 0.017 % bt709 when written), and no partial sum reaches
    1.45e8 (int32 holds 2.1e9). (Of the witness surface_ref.convert10, not of the kernel: see the head of this file.)"""
    grid = np.asarray(sorted(set(range(0, 1024, 16)) | {63, 64, 511, 512, 513, 960, 961, 1023}))
    assert grid.size == 69
    cb, cr = grid[:, None], grid[None, :]
    worst, differ, bound, points = 0, 0, 0, 0
    for y in range(1024):
        got, b = S.convert10(np.full((1, 1), y), cb, cr, standard)
        bound = max(bound, b)
        for g, w in zip(got, S.exact10(np.full((1, 1), y), cb, cr, standard)):
            d = np.abs(np.broadcast_to(g, (69, 69)) - np.broadcast_to(w, (69, 69)))
            worst = max(worst, int(d.max()))
            differ += int((d != 0).sum())
        points += 69 * 69
    assert points == 4875264
    share = differ / (3 * points)
    print(f"{standard}: max |int - float64| = {worst}, differing share = {100 * share:.4f} %, largest partial sum = {bound}")
    assert worst <= 1
    assert share <= 0.001
    assert bound < 1.45e8


def test_low_six_bits_are_ignored():
    rng = np.random.RandomState(1)
    layout = P.SurfaceLayout((8, 12), "p010", pitch=32, luma_rows=10)
    frame = rng.randint(0, 256, (2, 12, 12)).astype(np.uint8)
    clean, dirty = S.to_p010(frame, 0), S.to_p010(frame, rng)
    assert (clean & 63).max() == 0 and (dirty & 63).max() == 63 and np.array_equal(clean >> 6, dirty >> 6)
    for standard in STANDARDS10:
        a = S.p010_to_bgr(S.pack(clean, layout, 0), layout, standard)
        b = S.p010_to_bgr(S.pack(dirty, layout, rng), layout, standard)
        assert np.array_equal(a, b)
        assert np.array_equal(a, Y.yuv420sp_to_bgr(frame, standard))     # (the lifted frame is the 8-bit picture)


# ------------------------------------------------------------------------------------------------------- SurfaceLayout
def test_layout_defaults_tight_and_key():
    hs, ws = 64, 96
    for fmt, row, shape in (("bgr", 288, (64, 96, 3)), ("nv12", 96, (96, 96)), ("nv21", 96, (96, 96)), ("p010", 192, (96, 192))):
        t = P.SurfaceLayout((hs, ws), fmt)
        assert t.tight and t.key is None and t.pitch == row == t.row_bytes
        assert t.image_bytes == t.sample_end == int(np.prod(shape)) == int(np.prod(P.frame_shape((hs, ws), fmt)))
        if fmt != "bgr":
            assert (t.luma_rows, t.chroma_pitch, t.chroma_offset) == (hs, row, hs * row)
    pad = P.SurfaceLayout((hs, ws), "nv12", pitch=128, luma_rows=80)
    assert not pad.tight and (pad.chroma_pitch, pad.chroma_offset) == (128, 80 * 128)
    assert pad.sample_end == 80 * 128 + 31 * 128 + 96 == pad.image_bytes
    assert pad.key == (128, 80, 128, 80 * 128, pad.image_bytes)
    own = P.SurfaceLayout((hs, ws), "nv12", pitch=128, luma_rows=80, chroma_pitch=112, chroma_offset=80 * 128 + 4, image_bytes=20000)
    assert own.sample_end == 80 * 128 + 4 + 31 * 112 + 96 and own.image_bytes == 20000 and own.key != pad.key
    # a field given its default value is still a given field: not the tight form's key, but the same bytes
    same = P.SurfaceLayout((hs, ws), "nv12", pitch=96)
    assert not same.tight and same.image_bytes == 96 * 96
    assert P.SurfaceLayout((30, 50), "bgr", pitch=151).sample_end == 29 * 151 + 150
    p = P.SurfaceLayout((hs, ws), "p010", pitch=256, luma_rows=80)
    assert (p.row_bytes, p.chroma_offset, p.sample_end) == (192, 80 * 256, 80 * 256 + 31 * 256 + 192)
    # the dict form and the checked pass-through
    assert P.SurfaceLayout.make(dict(pitch=128, luma_rows=80), (hs, ws), "nv12").key == pad.key
    assert P.SurfaceLayout.make(pad, (hs, ws), "nv12") is pad and P.SurfaceLayout.make(None, (hs, ws), "nv12").tight
    with pytest.raises(ValueError, match="does not describe"):
        P.SurfaceLayout.make(pad, (hs, ws), "nv21")


@pytest.mark.parametrize("fmt,kw,words", [
    ("nv12", dict(pitch=95), "rows overlap"),
    ("bgr", dict(pitch=287), "rows overlap"),
    ("p010", dict(pitch=190), "rows overlap"),
    ("nv12", dict(chroma_pitch=90), "chroma rows overlap"),
    ("nv12", dict(luma_rows=62), "luma_rows 62"),
    ("nv12", dict(pitch=128, chroma_offset=63 * 128 + 95), "planes overlap"),
    ("nv12", dict(chroma_offset=0), "planes overlap"),
    ("p010", dict(pitch=193), "even"),
    ("p010", dict(chroma_pitch=193), "even"),
    ("p010", dict(chroma_offset=64 * 192 + 1), "even"),
    ("p010", dict(image_bytes=96 * 192 + 1), "even"),
    ("nv12", dict(image_bytes=96 * 96 - 1), "outside image_bytes"),
    ("nv12", dict(pitch=128, image_bytes=96 * 96), "outside image_bytes"),
    ("bgr", dict(image_bytes=64 * 288 - 1), "outside image_bytes"),
    ("bgr", dict(luma_rows=80), "one plane"),
    ("bgr", dict(chroma_pitch=288), "one plane"),
    ("bgr", dict(chroma_offset=64 * 288), "one plane"),
])
def test_layout_refusals_name_the_layout(fmt, kw, words):
    with pytest.raises(ValueError, match=words) as err:
        P.SurfaceLayout((64, 96), fmt, **kw)
    if "one plane" not in words:
        assert f"{fmt} surface of 96 x 64" in str(err.value)


def test_layout_refusals_of_formats_and_colours():
    with pytest.raises(ValueError, match="frame format"):
        P.SurfaceLayout((64, 96), "i420")
    with pytest.raises(ValueError, match="even"):
        P.SurfaceLayout((63, 96), "p010")
    with pytest.raises(ValueError, match="jfif"):
        P.ResamplePlan((64, 96), None, frame_format="p010")                  # (the default standard is the JPEG one)
    with pytest.raises(ValueError, match="jfif"):
        P.plan_key((64, 96), None, "p010", "jfif")
    with pytest.raises(ValueError, match="colour standard"):
        P.ResamplePlan((64, 96), None, frame_format="p010", colour="bt2020")
    with pytest.raises(ValueError, match="jfif"):
        P.p010_coefficients("jfif")
    for c in STANDARDS10:
        assert P.ResamplePlan((64, 96), None, frame_format="p010", colour=c).yuv == Y.integer_matrix(c)


def test_plan_keys_differ_by_layout_and_tight_is_todays():
    aug, hw = dict(resize=0.5), (64, 96)
    today = P.plan_key(hw, aug, "nv12", "bt601")
    assert len(today) == 7
    assert P.plan_key(hw, aug, "nv12", "bt601", P.SurfaceLayout(hw, "nv12")) == today
    assert P.plan_key(hw, aug, "nv12", "bt601", None) == today
    assert P.ResamplePlan(hw, aug, None, "nv12", "bt601", layout=P.SurfaceLayout(hw, "nv12")).key == today
    assert P.ResamplePlan(hw, aug, None, "nv12", "bt601").key == today
    layouts = [dict(pitch=128), dict(pitch=100), dict(luma_rows=80), dict(pitch=128, luma_rows=80),
               dict(pitch=128, luma_rows=80, chroma_pitch=112, chroma_offset=80 * 128 + 4), dict(image_bytes=96 * 96 + 1000)]
    keys = [P.plan_key(hw, aug, "nv12", "bt601", kw) for kw in layouts]
    assert len(set(keys + [today])) == len(layouts) + 1
    for kw, key in zip(layouts, keys):
        plan = P.ResamplePlan(hw, aug, None, "nv12", "bt601", layout=kw)
        assert plan.key == key and plan.frame_shape == (plan.surface.image_bytes,) and key[:7] == today
    assert P.plan_key(hw, aug, "p010", "bt601") != P.plan_key(hw, aug, "p010", "bt709") != today
    # a plan without a layout is what it was: shapes and the words of its refusals
    plain = P.ResamplePlan(hw, aug, None, "nv12", "bt601")
    assert plain.frame_shape == (96, 96) and plain.surface.tight and "a padded pitch is not taken" in plain.layout()
    assert P.ResamplePlan(hw, aug, None, "p010", "bt601").frame_shape == (96, 192)


def test_plan_words_and_bytes_of_the_new_forms():
    torch = pytest.importorskip("torch")
    hw, aug = (64, 96), dict(resize=1, crop=(0, 3, 96, 8))
    pad = P.ResamplePlan(hw, aug, None, "nv12", "bt601", layout=dict(pitch=128, luma_rows=80))
    assert "pitch 128 in a plane of 80" in pad.layout() and str(pad.surface.image_bytes) in pad.layout()
    for bad in (torch.zeros(1, 96, 96, dtype=torch.uint8), torch.zeros(pad.surface.image_bytes, dtype=torch.uint8),
                torch.zeros(1, pad.surface.image_bytes, dtype=torch.int8)):
        with pytest.raises(ValueError, match="nv12 surface of 96 x 64"):
            pad.run(bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        pad.run(torch.zeros(2, pad.surface.image_bytes, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="host memory"):
        pad.run_surfaces([torch.zeros(pad.surface.image_bytes, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="one device u8 tensor per image"):
        pad.run_surfaces([torch.zeros(pad.surface.image_bytes, dtype=torch.int16)])
    with pytest.raises(ValueError, match="empty"):
        pad.run_surfaces([])
    p10 = P.ResamplePlan(hw, aug, None, "p010", "bt709")
    with pytest.raises(ValueError, match=r"96, 192\] p010 frames"):
        p10.run(torch.zeros(1, 96, 96, dtype=torch.uint8))
    # the sample bytes actually read: 5 luma rows and the 3 chroma rows under them, whatever the pitch
    assert (pad.src_row0, pad.src_rows) == (3, 5)
    assert pad.bytes_per_image(288)["source"] == 8 * 96 == P.ResamplePlan(hw, aug, None, "nv12").bytes_per_image(288)["source"]
    assert p10.bytes_per_image(288)["source"] == 8 * 192
    assert P.ResamplePlan(hw, aug, None, layout=dict(pitch=300)).bytes_per_image(288)["source"] == 5 * 288


# ------------------------------------------------------------------------------------------------------- pack / unpack
@pytest.mark.parametrize("fmt,kw", [("nv12", dict(pitch=128, luma_rows=80, chroma_pitch=112, chroma_offset=80 * 128 + 4, image_bytes=16000)),
                                    ("nv21", dict(pitch=100)), ("bgr", dict(pitch=301, image_bytes=20000)),
                                    ("p010", dict(pitch=202, luma_rows=66)), ("nv12", dict())])
def test_pack_round_trips(fmt, kw):
    rng = np.random.RandomState(3)
    layout = P.SurfaceLayout((64, 96), fmt, **kw)
    shape = (2, 64, 96, 3) if fmt == "bgr" else (2, 96, 96)
    frame = rng.randint(0, 65536 if fmt == "p010" else 256, shape).astype(np.uint16 if fmt == "p010" else np.uint8)
    mask = S.sample_mask(layout)
    assert int(mask.sum()) == frame[0].size * frame.itemsize and mask[layout.sample_end - 1] and not mask[layout.sample_end:].any()
    a, b = S.pack(frame, layout, 0xFF), S.pack(frame, layout, rng)
    assert a.shape == (2, layout.image_bytes) and a.dtype == np.uint8
    assert np.array_equal(S.unpack(a, layout), frame) and np.array_equal(S.unpack(b, layout), frame)
    assert (a[:, ~mask] == 0xFF).all() and np.array_equal(a[:, mask], b[:, mask])
    if layout.tight:
        assert np.array_equal(a.reshape(frame.shape), frame)


# ------------------------------------------------------------------------------------------------------- the C entry
def test_c_entry_refuses_bad_arguments_before_any_hip_call():
    """As tests/test_capi.py: validation precedes any HIP call, so it is checkable without a device."""
    from simpb_amd import _lib
    fn = _lib.lib().simpb_preprocess_surface_nhwc4_f16
    null, ok = ctypes.c_void_p(0), ctypes.c_void_p(64)
    ints = dict(num_images=2, src_height=64, src_width=96, out_height=32, out_width=48, taps_x=9, taps_y=9, src_row0=0, src_rows=64,
                flip=0, swap_rb=1, format=1, pitch=128, chroma_pitch=112, chroma_offset=80 * 128 + 4, image_stride=16000,
                yoff=16, iy=76309, irv=104597, igu=-25675, igv=-53279, ibu=132201)
    names = ["out", "src", "image_table", "mid", "kx", "xlo", "xn", "ky", "ylo", "yn", "lut"]

    def call(ptrs=None, **changed):
        vals = dict(ints, **changed)
        p = dict(dict.fromkeys(names, ok), image_table=null)
        p.update(ptrs or {})
        return fn(*[p[k] for k in names], *vals.values(), null)

    for k in names:
        if k != "image_table":
            assert call({k: null}) == 1, k
    assert call(dict(src=ok, image_table=ok)) == 1                                  # both forms of the images
    assert call(dict(src=null, image_table=null)) == 1                              # neither
    assert call(dict(src=null, image_table=ctypes.c_void_p(68))) == 1               # a table of 64-bit words
    assert call(format=4) == 1 and call(format=-1) == 1
    assert call(pitch=95) == 1 and call(chroma_pitch=95) == 1                       # below the row's sample bytes
    assert call(format=0, pitch=287) == 1 and call(format=3, pitch=190, chroma_pitch=192) == 1
    assert call(chroma_offset=63 * 128 + 95) == 1 and call(chroma_offset=-1) == 1   # the planes overlap
    last = 80 * 128 + 4 + 31 * 112 + 96
    assert call(image_stride=last - 1) == 1                                         # the last sample outside the image
    assert call(format=0, pitch=300, image_stride=63 * 300 + 287) == 1
    p010 = dict(format=3, pitch=256, chroma_pitch=256, chroma_offset=80 * 256, image_stride=30000)
    for k in ("pitch", "chroma_pitch", "chroma_offset", "image_stride"):
        assert call(**dict(p010, **{k: p010[k] + 1})) == 1, k                       # odd values for 16-bit samples
    assert call(dict(src=ctypes.c_void_p(65)), **p010) == 1
    # what the older entries refuse is refused as well
    assert call(src_height=65, src_rows=65) == 1 and call(src_width=97) == 1 and call(iy=0) == 1
    assert call(num_images=0) == 1 and call(src_width=4098) == 1 and call(out_width=2049) == 1 and call(taps_x=65) == 1
    assert call(src_row0=1) == 1 and call(dict(out=ctypes.c_void_p(72))) == 1
