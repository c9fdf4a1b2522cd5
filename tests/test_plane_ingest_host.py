"""CPU: the host side of the plane ingest -- planar 4:2:0 ("yuv420p" / "yvu420p"), packed 4:2:2 ("yuyv" / "uyvy") and the RGB-order
family ("rgb" / "bgra" / "rgba"): SurfaceLayout's defaults, keys, words and refusals (simpb_amd/preprocess.py), the witness's
pack / unpack (tests/planes_ref.py), the rig descriptors, and the argument checks of simpb_preprocess_planes_nhwc4_f16 and of the
rig entry, which run before any HIP call."""
import ctypes

import numpy as np
import pytest

from simpb_amd import _lib
from simpb_amd import preprocess as P
from tests import planes_ref as L
from tests import yuv_ref as Y

HW = (64, 96)


# ------------------------------------------------------------------------------------------------------- names and shapes
def test_names_codes_and_shapes():
    assert P.FRAME_FORMATS[:4] == ("bgr", "nv12", "nv21", "p010") and set(P.FRAME_FORMATS[4:]) == set(L.NEW)
    assert [P.SURFACE_FORMAT[f] for f in ("bgr", "nv12", "nv21", "p010")] == [0, 1, 2, 3]
    assert [P.SURFACE_FORMAT[f] for f in ("yuv420p", "yvu420p", "yuyv", "uyvy", "rgb", "bgra", "rgba")] == [8, 8, 9, 10, 11, 12, 13]
    shapes = dict(yuv420p=(96, 96), yvu420p=(96, 96), yuyv=(64, 96, 2), uyvy=(64, 96, 2), rgb=(64, 96, 3), bgra=(64, 96, 4), rgba=(64, 96, 4))
    for fmt, shape in shapes.items():
        assert P.frame_shape(HW, fmt) == shape
        plan = P.ResamplePlan(HW, dict(resize=0.5), None, fmt)
        assert plan.frame_shape == shape and plan.surface.tight and plan.surface.image_bytes == int(np.prod(shape))
        assert (plan.yuv is None) == (fmt in ("rgb", "bgra", "rgba"))
    assert P.frame_shape(HW, "yuv420p") == P.frame_shape(HW, "nv12")      # a caller's NV12 buffers carry over
    assert P.frame_shape((31, 50), "uyvy") == (31, 50, 2) and P.frame_shape((31, 51), "rgba") == (31, 51, 4)
    for fmt, hw in (("yuv420p", (63, 96)), ("yvu420p", (64, 95)), ("yuyv", (64, 95)), ("uyvy", (31, 51))):
        with pytest.raises(ValueError, match="even"):
            P.frame_shape(hw, fmt)
        with pytest.raises(ValueError, match="even"):
            P.SurfaceLayout(hw, fmt)


def test_i420_is_still_no_name():
    for make in (lambda: P.SurfaceLayout(HW, "i420"), lambda: P.ResamplePlan(HW, None, frame_format="i420"),
                 lambda: P.CameraSource(HW, None, "i420"), lambda: P.plan_key(HW, None, "i420")):
        with pytest.raises(ValueError, match="frame format") as err:
            make()
        assert "'yuv420p'" in str(err.value) and "'yvu420p'" in str(err.value)


# ------------------------------------------------------------------------------------------------------- SurfaceLayout
def test_planar_defaults_of_both_names():
    for fmt in L.PLANAR:
        t = P.SurfaceLayout(HW, fmt)
        assert t.tight and t.key is None and (t.pitch, t.chroma_pitch, t.luma_rows) == (96, 48, 64)
        cb, cr = (64 * 96, 64 * 96 + 32 * 48) if fmt == "yuv420p" else (64 * 96 + 32 * 48, 64 * 96)
        assert (t.chroma_offset, t.chroma2_offset) == (cb, cr) and t.sample_end == t.image_bytes == 96 * 96
        pad = P.SurfaceLayout(HW, fmt, pitch=128, luma_rows=80)
        first, second = 80 * 128, 80 * 128 + 32 * 64
        assert pad.chroma_pitch == 64
        assert (pad.chroma_offset, pad.chroma2_offset) == ((first, second) if fmt == "yuv420p" else (second, first))
        assert pad.sample_end == second + 31 * 64 + 48 == pad.image_bytes
        assert pad.key == (128, 80, 64, pad.chroma_offset, pad.image_bytes, pad.chroma2_offset)
    # given offsets mean the same for both names: chroma_offset is Cb, chroma2_offset is Cr
    kw = dict(pitch=100, chroma_pitch=51, chroma_offset=64 * 100 + 7, chroma2_offset=64 * 100 + 7 + 32 * 51 + 3, image_bytes=12000)
    a, b = P.SurfaceLayout(HW, "yuv420p", **kw), P.SurfaceLayout(HW, "yvu420p", **kw)
    assert a.key == b.key and (a.chroma_offset, a.chroma2_offset) == (b.chroma_offset, b.chroma2_offset) == (6407, 6407 + 32 * 51 + 3)
    assert a.sample_end == 6407 + 32 * 51 + 3 + 31 * 51 + 48
    # Cr in front of Cb by hand is the other name's default
    swapped = P.SurfaceLayout(HW, "yuv420p", chroma_offset=64 * 96 + 32 * 48, chroma2_offset=64 * 96)
    other = P.SurfaceLayout(HW, "yvu420p")
    assert (swapped.chroma_offset, swapped.chroma2_offset, swapped.image_bytes) == (other.chroma_offset, other.chroma2_offset, other.image_bytes)
    with pytest.raises(ValueError, match="yuv420p surface of 50 x 30.*odd"):
        P.SurfaceLayout((30, 50), "yuv420p", pitch=55)
    odd = P.SurfaceLayout((30, 50), "yuv420p", pitch=55, chroma_pitch=27)
    assert (odd.chroma_offset, odd.chroma2_offset, odd.sample_end) == (30 * 55, 30 * 55 + 15 * 27, 30 * 55 + 15 * 27 + 14 * 27 + 25)


def test_packed_defaults():
    for fmt, px in (("yuyv", 2), ("uyvy", 2), ("rgb", 3), ("bgra", 4), ("rgba", 4)):
        t = P.SurfaceLayout(HW, fmt)
        assert t.tight and t.key is None and t.pitch == t.row_bytes == 96 * px and t.image_bytes == t.sample_end == 64 * 96 * px
        assert (t.luma_rows, t.chroma_pitch, t.chroma_offset, t.chroma2_offset) == (64, 0, 0, 0)
        pad = P.SurfaceLayout((31, 50), fmt, pitch=50 * px + 3, image_bytes=31 * (50 * px + 3) + 9)
        assert pad.sample_end == 30 * (50 * px + 3) + 50 * px and pad.key == (50 * px + 3, 31, 0, 0, pad.image_bytes)


@pytest.mark.parametrize("fmt,kw,words", [
    ("yuv420p", dict(pitch=94), "rows overlap"),
    ("yvu420p", dict(chroma_pitch=47), "chroma rows overlap"),
    ("yuv420p", dict(luma_rows=62), "luma_rows 62"),
    ("yuv420p", dict(chroma_offset=64 * 96 - 1), "planes overlap"),
    ("yuv420p", dict(chroma2_offset=63 * 96 + 95), "planes overlap"),
    ("yuv420p", dict(chroma2_offset=64 * 96 + 32 * 48 - 1), "planes overlap"),            # Cr starts inside Cb
    ("yvu420p", dict(chroma_offset=64 * 96 + 31 * 48 + 47), "planes overlap"),            # Cb starts inside Cr
    ("yuv420p", dict(chroma_offset=64 * 96, chroma2_offset=64 * 96), "planes overlap"),
    ("yuv420p", dict(image_bytes=96 * 96 - 1), "outside image_bytes"),
    ("yvu420p", dict(pitch=128, image_bytes=96 * 96), "outside image_bytes"),
    ("yuyv", dict(pitch=191), "rows overlap"),
    ("uyvy", dict(image_bytes=64 * 192 - 1), "outside image_bytes"),
    ("rgb", dict(pitch=287), "rows overlap"),
    ("bgra", dict(pitch=383), "rows overlap"),
    ("rgba", dict(image_bytes=64 * 384 - 1), "outside image_bytes"),
    ("yuyv", dict(luma_rows=80), "one plane"),
    ("uyvy", dict(chroma_pitch=96), "one plane"),
    ("rgb", dict(chroma_offset=64 * 288), "one plane"),
    ("bgra", dict(chroma2_offset=64 * 384), "one plane"),
    ("bgr", dict(chroma2_offset=64 * 288), "one plane"),
    ("nv12", dict(chroma2_offset=64 * 96), "must not be given"),
    ("p010", dict(chroma2_offset=64 * 192), "must not be given"),
])
def test_layout_refusals_name_the_layout(fmt, kw, words):
    with pytest.raises(ValueError, match=words) as err:
        P.SurfaceLayout(HW, fmt, **kw)
    if "one plane" in words or "must not be given" in words:
        assert f"a {fmt} surface" in str(err.value) and "must not be given" in str(err.value)
    else:
        assert f"{fmt} surface of 96 x 64" in str(err.value)


def test_keys():
    aug = dict(resize=0.5)
    # the four first formats keep their keys, with and without a layout
    old = {("bgr", None): (64, 96, (48, 32), (0, 0, 48, 32), False, "bgr", None),
           ("nv12", None): (64, 96, (48, 32), (0, 0, 48, 32), False, "nv12", "bt601"),
           ("nv12", 128): (64, 96, (48, 32), (0, 0, 48, 32), False, "nv12", "bt601", (128, 64, 128, 64 * 128, 64 * 128 + 31 * 128 + 96)),
           ("p010", 256): (64, 96, (48, 32), (0, 0, 48, 32), False, "p010", "bt601", (256, 64, 256, 64 * 256, 64 * 256 + 31 * 256 + 192)),
           ("bgr", 300): (64, 96, (48, 32), (0, 0, 48, 32), False, "bgr", None, (300, 64, 0, 0, 63 * 300 + 288))}
    for (fmt, pitch), key in old.items():
        assert P.plan_key(HW, aug, fmt, "bt601", None if pitch is None else dict(pitch=pitch)) == key
    # the colour standard is left out of the key of the RGB-order formats, and is part of the YCbCr ones'
    for fmt in ("rgb", "bgra", "rgba"):
        assert P.plan_key(HW, aug, fmt, "bt601") == P.plan_key(HW, aug, fmt, "bt709") == (64, 96, (48, 32), (0, 0, 48, 32), False, fmt, None)
    for fmt in ("yuv420p", "yvu420p", "yuyv", "uyvy"):
        assert P.plan_key(HW, aug, fmt, "bt601") != P.plan_key(HW, aug, fmt, "bt709")
        assert P.plan_key(HW, aug, fmt, "bt601", P.SurfaceLayout(HW, fmt)) == P.plan_key(HW, aug, fmt, "bt601") and len(P.plan_key(HW, aug, fmt)) == 7
    assert len({P.plan_key(HW, aug, fmt) for fmt in P.FRAME_FORMATS if fmt != "p010"}) == 10
    # distinct per field
    fields = [dict(pitch=128), dict(luma_rows=80), dict(chroma_pitch=50), dict(chroma_offset=64 * 96 + 32 * 48 + 32 * 48),
              dict(chroma2_offset=64 * 96 + 32 * 48 + 1), dict(image_bytes=96 * 96 + 100), dict(pitch=96)]
    keys = [P.plan_key(HW, aug, "yuv420p", "jfif", kw) for kw in fields]
    assert len(set(keys + [P.plan_key(HW, aug, "yuv420p")])) == len(fields) + 1
    for fmt in ("yuyv", "rgb", "rgba"):
        px = P.PIXEL_BYTES[fmt]
        keys = [P.plan_key(HW, aug, fmt, "jfif", kw) for kw in (dict(pitch=96 * px + 1), dict(image_bytes=64 * 96 * px + 1), dict(pitch=96 * px))]
        assert len(set(keys + [P.plan_key(HW, aug, fmt)])) == 4


def test_words_and_bytes():
    hw, aug = HW, dict(resize=1, crop=(0, 3, 96, 8))
    plans = {fmt: P.ResamplePlan(hw, aug, None, fmt) for fmt in L.NEW}
    assert all((p.src_row0, p.src_rows) == (3, 5) for p in plans.values())
    # 5 luma rows and the chroma rows 1 .. 3 of both planes; 4:2:2 rows carry their own chroma; alpha bytes count as read
    want = dict(yuv420p=5 * 96 + 2 * 3 * 48, yvu420p=5 * 96 + 2 * 3 * 48, yuyv=5 * 192, uyvy=5 * 192, rgb=5 * 288, bgra=5 * 384, rgba=5 * 384)
    for fmt, p in plans.items():
        assert p.bytes_per_image(288)["source"] == want[fmt], fmt
        assert fmt in p.layout() and fmt in p.surface.describe()
    assert plans["yuv420p"].bytes_per_image(288)["source"] == P.ResamplePlan(hw, aug, None, "nv12").bytes_per_image(288)["source"]
    assert "Cb plane, then the Cr plane" in plans["yuv420p"].layout() and "Cr plane, then the Cb plane" in plans["yvu420p"].layout()
    assert "[..., 64, 96, 2]" in plans["uyvy"].layout() and "(Cb, Y0, Cr, Y1)" in plans["uyvy"].layout()
    assert "[..., 64, 96, 4]" in plans["rgba"].layout()
    pad = P.ResamplePlan(hw, aug, None, "yvu420p", layout=dict(pitch=128, luma_rows=80))
    assert pad.bytes_per_image(288)["source"] == want["yvu420p"]
    d = pad.surface.describe()
    assert "pitch 128 in a plane of 80" in d and f"Cb from byte {80 * 128 + 32 * 64}" in d and f"Cr from byte {80 * 128}" in d
    assert d in pad.layout() and "chroma2_offset=10240" in repr(pad.surface)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="yvu420p surface of 96 x 64"):
        pad.run(torch.zeros(1, 96, 96, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"64, 96, 2\] yuyv frames"):
        plans["yuyv"].run(torch.zeros(1, 64, 96, 3, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------- the witness
@pytest.mark.parametrize("fmt,hw,kw", [
    ("yuv420p", (30, 50), dict(pitch=55, chroma_pitch=27, image_bytes=3000)),          # an odd chroma pitch at Ws 50, tail padding
    ("yvu420p", (30, 50), dict(pitch=64, luma_rows=32)),
    ("yuv420p", HW, dict(pitch=100, chroma_pitch=51, chroma_offset=64 * 100 + 7, chroma2_offset=64 * 100 + 7 + 32 * 51 + 3)),
    ("yvu420p", HW, dict()),
    ("yuyv", (31, 50), dict(pitch=103, image_bytes=4000)), ("uyvy", HW, dict()),
    ("rgb", (31, 50), dict(pitch=151)), ("bgra", (31, 50), dict(pitch=203, image_bytes=7000)), ("rgba", HW, dict())])
def test_pack_round_trips(fmt, hw, kw):
    rng = np.random.RandomState(3)
    layout = P.SurfaceLayout(hw, fmt, **kw)
    frame = rng.randint(0, 256, (2,) + P.frame_shape(hw, fmt)).astype(np.uint8)
    mask = L.sample_mask(layout)
    assert int(mask.sum()) == frame[0].size and mask[layout.sample_end - 1] and not mask[layout.sample_end:].any()
    a, b = L.pack(frame, layout, 0xFF), L.pack(frame, layout, rng)
    assert a.shape == (2, layout.image_bytes) and a.dtype == np.uint8
    assert np.array_equal(L.unpack(a, layout), frame) and np.array_equal(L.unpack(b, layout), frame)
    assert (a[:, ~mask] == 0xFF).all() and np.array_equal(a[:, mask], b[:, mask])
    if layout.tight:
        assert np.array_equal(a.reshape(frame.shape), frame)
    if fmt in L.PLANAR:      # the planes lie where the layout says, Cb at chroma_offset under either name
        luma, cb, cr = L.planes(frame, fmt)
        for i in (0, hw[0] // 2 - 1):
            at, at2 = layout.chroma_offset + i * layout.chroma_pitch, layout.chroma2_offset + i * layout.chroma_pitch
            assert np.array_equal(a[:, at:at + hw[1] // 2], cb[:, i]) and np.array_equal(a[:, at2:at2 + hw[1] // 2], cr[:, i])


def test_witness_pictures_agree_across_formats():
    """The same samples in every YCbCr arrangement give one picture, and the RGB family one picture: the builders and to_bgr."""
    rng = np.random.RandomState(4)
    nv12 = rng.randint(0, 256, (2, 96, 96)).astype(np.uint8)
    for standard in ("jfif", "bt601", "bt709"):
        bgr = Y.yuv420sp_to_bgr(nv12, standard)
        for fmt in L.PLANAR:
            planar = L.planar_from_nv12(nv12, fmt)
            assert np.array_equal(L.to_bgr(planar, fmt, standard), bgr) and np.array_equal(L.nv12_from_planar(planar, fmt), nv12)
        assert not np.array_equal(L.to_bgr(L.planar_from_nv12(nv12, "yuv420p"), "yvu420p", standard), bgr)
        # 4:2:2 whose chroma rows repeat in pairs is the 4:2:0 picture
        luma, cb, cr = L.planes(L.planar_from_nv12(nv12, "yuv420p"), "yuv420p")
        yuyv = L.packed_422(luma, np.repeat(cb, 2, axis=-2), np.repeat(cr, 2, axis=-2), "yuyv")
        assert np.array_equal(L.to_bgr(yuyv, "yuyv", standard), bgr)
        assert np.array_equal(L.to_bgr(L.swap_422(yuyv), "uyvy", standard), bgr)
    pic = rng.randint(0, 256, (2, 31, 50, 3)).astype(np.uint8)
    for fmt in ("rgb", "bgra", "rgba"):
        assert np.array_equal(L.to_bgr(L.from_bgr(pic, fmt, rng), fmt), pic)
    assert np.array_equal(L.from_bgr(pic, "rgba", 9)[..., 0], pic[..., 2]) and (L.from_bgr(pic, "bgra", 9)[..., 3] == 9).all()


# ------------------------------------------------------------------------------------------------------- the rig
def rig_sources():
    return [P.CameraSource((64, 96), dict(resize=0.5, crop=(4, 4, 44, 28))),
            P.CameraSource((100, 168), dict(resize=0.25, crop=(1, 1, 41, 25)), "nv12", layout=dict(pitch=176)),
            P.CameraSource((64, 96), dict(resize=0.5, crop=(0, 0, 40, 24)), "yuv420p", "bt601", dict(pitch=112, luma_rows=72, chroma_pitch=60)),
            P.CameraSource((31, 50), dict(resize=1, crop=(5, 3, 45, 27), flip=True), "uyvy", "bt709", dict(pitch=103)),
            P.CameraSource((12, 20), dict(resize=2, crop=(0, 0, 40, 24)), "bgra")]


def test_descriptors_carry_the_new_fields():
    rig = P.RigPlan(rig_sources())
    cams = rig.descriptors()
    assert ctypes.sizeof(_lib.RigCamera) == 112 and _lib.RigCamera.chroma2_offset.offset == 104
    assert [c.format for c in cams] == [0, 1, 8, 10, 12]
    for c, sf in zip(cams, rig.surfaces):
        assert (c.pitch, c.chroma_pitch, c.chroma_offset, c.chroma2_offset) == (sf.pitch, sf.chroma_pitch, sf.chroma_offset, sf.chroma2_offset)
    assert (cams[2].chroma_offset, cams[2].chroma2_offset, cams[2].chroma_pitch) == (72 * 112, 72 * 112 + 32 * 60, 60)
    assert [c.chroma2_offset for c in cams[:2] + cams[3:]] == [0, 0, 0, 0] and (cams[3].pitch, cams[4].pitch) == (103, 80)
    assert (cams[2].yoff, cams[2].iy) == P.yuv_coefficients("bt601")[:2] and cams[3].iy == P.yuv_coefficients("bt709")[1] and cams[4].iy == 1
    assert P.RigPlan(rig_sources()).key == rig.key
    other = rig_sources()
    other[2] = P.CameraSource((64, 96), dict(resize=0.5, crop=(0, 0, 40, 24)), "yvu420p", "bt601", dict(pitch=112, luma_rows=72, chroma_pitch=60))
    assert P.RigPlan(other).key != rig.key


def test_rig_entry_point_refuses_bad_cameras_before_any_hip_call():
    rig = P.RigPlan(rig_sources())
    fn = _lib.lib().simpb_preprocess_rig_nhwc4_f16
    one = ctypes.c_void_p(64)
    lens = (sum(k.size for k in rig.kx), 5 * 40, sum(k.size for k in rig.ky), 5 * 24, rig.mid_rows)

    def call(changed):
        cams = rig.descriptors()
        for (c, field), v in changed.items():
            setattr(cams[c], field, v)
        return fn(one, one, one, one, one, one, one, one, one, one, cams, 5, 10, 24, 40, *lens, 1, None)

    sf = rig.surfaces[2]
    bad = [{(2, "chroma2_offset"): sf.chroma_offset}, {(2, "chroma2_offset"): sf.chroma_offset + 31 * 60 + 47},     # Cb / Cr overlap
           {(2, "chroma2_offset"): 63 * 112 + 95}, {(2, "chroma_pitch"): 47}, {(2, "src_width"): 94 + 1},
           {(3, "src_width"): 49}, {(3, "pitch"): 99}, {(4, "pitch"): 79}, {(3, "iy"): 0},
           {(0, "format"): 6}, {(4, "format"): 4}, {(4, "format"): 7}, {(4, "format"): 14}, {(4, "format"): -1}]
    for changed in bad:
        assert call(changed) == 1, changed


# ------------------------------------------------------------------------------------------------------- the C entry
def test_c_entry_refuses_bad_arguments_before_any_hip_call():
    """As tests/test_capi.py: validation precedes any HIP call, so it is checkable without a device. Every call below is refused;
    the base arguments are a consistent padded yuv420p batch, so each refusal has the one cause its line names."""
    fn = _lib.lib().simpb_preprocess_planes_nhwc4_f16
    null, ok = ctypes.c_void_p(0), ctypes.c_void_p(64)
    cb, cr = 80 * 128 + 4, 80 * 128 + 4 + 32 * 56
    last = cr + 31 * 56 + 48
    ints = dict(num_images=2, src_height=64, src_width=96, out_height=32, out_width=48, taps_x=9, taps_y=9, src_row0=0, src_rows=64,
                flip=0, swap_rb=1, format=8, pitch=128, chroma_pitch=56, chroma_offset=cb, chroma2_offset=cr, image_stride=last,
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
    assert call(dict(src=ok, image_table=ok)) == 1 and call(dict(src=null, image_table=null)) == 1
    assert call(dict(src=null, image_table=ctypes.c_void_p(68))) == 1
    for code in (4, 5, 6, 7, 14, -1):
        assert call(format=code) == 1, code
    assert call(src_height=65, src_rows=65) == 1 and call(src_width=97) == 1 and call(iy=0) == 1
    assert call(pitch=95) == 1 and call(chroma_pitch=47) == 1                          # below the rows' sample bytes
    assert call(chroma_offset=63 * 128 + 95) == 1 and call(chroma2_offset=63 * 128 + 95) == 1 and call(chroma2_offset=-1) == 1
    assert call(chroma2_offset=cb) == 1 and call(chroma2_offset=cb + 31 * 56 + 47) == 1      # the chroma planes overlap
    assert call(chroma_offset=cr + 31 * 56 + 47, image_stride=30000) == 1                    # ... the other way round
    assert call(image_stride=last - 1) == 1                                                   # the last sample outside the image
    assert call(chroma_offset=cr + 32 * 56, image_stride=cr + 32 * 56 + 31 * 56 + 47) == 1     # ... when Cb is the last plane
    one_plane = dict(chroma_pitch=0, chroma_offset=0, chroma2_offset=0)
    for code, px in ((9, 2), (10, 2), (11, 3), (12, 4), (13, 4)):
        base = dict(one_plane, format=code, pitch=96 * px + 5, image_stride=63 * (96 * px + 5) + 96 * px)
        assert call(**dict(base, pitch=96 * px - 1)) == 1, code
        assert call(**dict(base, image_stride=base["image_stride"] - 1)) == 1, code
        assert call(**dict(base, src_width=4098)) == 1 and call(**dict(base, num_images=0)) == 1
    for code in (9, 10):
        assert call(**dict(one_plane, format=code, src_width=95, pitch=400, image_stride=64 * 400)) == 1     # an odd width for 4:2:2
        assert call(**dict(one_plane, format=code, pitch=400, image_stride=64 * 400, iy=0)) == 1
    # codes 0..3 are the older entry's, refusals included
    assert call(format=1, chroma_pitch=95, chroma2_offset=0) == 1 and call(format=0, pitch=287) == 1
    assert call(format=3, pitch=257, chroma_pitch=256, chroma_offset=80 * 256, chroma2_offset=0, image_stride=30000) == 1
    assert call(out_width=2049) == 1 and call(taps_x=65) == 1 and call(src_row0=1) == 1 and call(dict(out=ctypes.c_void_p(72))) == 1
