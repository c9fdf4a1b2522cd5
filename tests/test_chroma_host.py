"""CPU: the host side of the JPEG-decoder planes -- interpolated chroma (chroma="jpeg"), libjpeg's colour constants
(colour="jpeg") and planar 4:4:4 ("yuv444p"). The witness (tests/chroma_ref.py) against libjpeg through Pillow
(tests/golden/jpeg_chroma.npz, tools/golden/gen_jpeg_chroma_golden.py), byte for byte; the names, keys, layouts and words of
simpb_amd/preprocess.py and the runners; and the refusals of the C entry points, which run before any HIP call.

Pinned to libjpeg here: 4:2:0 (h2v2), 4:4:4 and the colour constants. The 4:2:2 rule (h2v1) is stated from libjpeg's published
algorithm and checked against a second statement only: libjpeg hands out no native planes of a 4:2:2 file."""
import ctypes
import functools
import importlib.util
import os
import types

import numpy as np
import pytest

from simpb_amd import _lib
from simpb_amd import preprocess as P
from tests import chroma_ref as C
from tests.helpers import load_golden

SIZES = ((2, 2), (6, 10), (18, 34), (32, 48))
HW = (64, 96)
JPEG = (0, 65536, 91881, -22554, -46802, 116130)
FLAG = 0x100


def files():
    g = load_golden("jpeg_chroma.npz")
    for sub in (2, 0):
        for h, w in SIZES:
            name = f"s{sub}_{h}x{w}"
            yield sub, (h, w), tuple(g[f"{name}_{k}"] for k in ("y", "cb", "cr", "rgb"))


def disagreeing_pairs():
    cb, cr = np.meshgrid(np.arange(256, dtype=np.int64) - 128, np.arange(256, dtype=np.int64) - 128, indexing="ij")
    return ((32768 - 22553 * cb - 46802 * cr) >> 16) != ((32768 - 22554 * cb - 46802 * cr) >> 16)


# ---------------------------------------------------------------------------------------------------- the witness and libjpeg
def test_witness_equals_libjpeg_on_native_planes_and_jfif_does_not():
    pairs = disagreeing_pairs()
    assert int(pairs.sum()) == 59
    seen = 0
    for sub, (h, w), (y, cb, cr, rgb) in files():
        assert y.shape == (h, w) and rgb.shape == (h, w, 3) and cb.shape == cr.shape == ((h, w) if sub == 0 else (h // 2, w // 2))
        ucb, ucr = (cb, cr) if sub == 0 else (C.fancy(cb), C.fancy(cr))
        assert pairs[ucb, ucr].any(), (sub, h, w)          # the condition on the inputs: a pair at which the two colours differ
        bgr = C.convert(y, ucb, ucr, "jpeg")
        assert np.array_equal(bgr[..., ::-1], rgb), (sub, h, w)
        other = C.convert(y, ucb, ucr, "jfif")
        assert (other != bgr).any() and np.abs(other.astype(int) - bgr).max() == 1 and np.array_equal(other[..., ::2], bgr[..., ::2])
        # the same through the frame builders the GPU tests use
        frame, fmt = (C.frame444(y, cb, cr), "yuv444p") if sub == 0 else (C.nv12_frame(y, cb, cr), "nv12")
        assert np.array_equal(C.to_bgr(frame, fmt, "jpeg"), bgr)
        if sub == 2 and h > 2:      # replicated chroma is another picture
            rep = C.convert(y, np.repeat(np.repeat(cb, 2, 0), 2, 1), np.repeat(np.repeat(cr, 2, 0), 2, 1), "jpeg")
            assert (rep != bgr).mean() > 0.5
        seen += 1
    assert seen == 8


def test_fixture_regenerates_with_libjpeg_turbo():
    features = pytest.importorskip("PIL.features")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("the fixture's bytes are libjpeg-turbo's")
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "golden", "gen_jpeg_chroma_golden.py")
    spec = importlib.util.spec_from_file_location("gen_jpeg_chroma_golden", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.SIZES == SIZES
    g, new = load_golden("jpeg_chroma.npz"), gen.arrays()
    assert sorted(g.files) == sorted(new)
    for k, v in new.items():
        assert v.dtype == g[k].dtype and np.array_equal(v, g[k]), k


def h2v1_loop(c):
    """libjpeg's h2v1_fancy_upsample as it is written: the first and last columns apart, the others in a loop over samples."""
    h, w = c.shape
    out = np.zeros((h, 2 * w), np.uint8)
    for r in range(h):
        row = [int(v) for v in c[r]]
        if w == 1:
            out[r] = row[0]
            continue
        o = [row[0], (row[0] * 3 + row[1] + 2) >> 2]
        for k in range(1, w - 1):
            v = row[k] * 3
            o += [(v + row[k - 1] + 1) >> 2, (v + row[k + 1] + 2) >> 2]
        o += [(row[-1] * 3 + row[-2] + 1) >> 2, row[-1]]
        out[r] = o
    return out


def h2v2_loop(c):
    """The rule of the issue, sample by sample."""
    hc, wc = c.shape
    out = np.zeros((2 * hc, 2 * wc), np.uint8)
    for r in range(2 * hc):
        i = r >> 1
        far = min(max(i + (1 if r & 1 else -1), 0), hc - 1)
        s = [3 * int(c[i, k]) + int(c[far, k]) for k in range(wc)]
        for x in range(2 * wc):
            j = x >> 1
            out[r, x] = (3 * s[j] + s[max(j - 1, 0)] + 8) >> 4 if x % 2 == 0 else (3 * s[j] + s[min(j + 1, wc - 1)] + 7) >> 4
    return out


def test_upsamplers_equal_their_loopwise_statements():
    rng = np.random.RandomState(7)
    for shape in ((1, 1), (1, 2), (3, 5), (2, 1), (9, 17), (4, 24)):
        c = rng.randint(0, 256, shape).astype(np.uint8)
        c.flat[0], c.flat[-1] = 255, 0
        assert np.array_equal(C.h2v1(c), h2v1_loop(c)), shape
        assert np.array_equal(C.fancy(c), h2v2_loop(c)), shape
    flat = np.full((3, 4), 201, np.uint8)
    assert (C.h2v1(flat) == 201).all() and (C.fancy(flat) == 201).all()
    # the frame builders: a 4:2:2 frame of either byte order and the four 4:2:0 arrangements hold one picture each
    from tests import planes_ref as L
    luma = rng.randint(0, 256, (6, 10)).astype(np.uint8)
    cb, cr = rng.randint(0, 256, (2, 6, 5)).astype(np.uint8)
    want = C.convert(luma, C.h2v1(cb), C.h2v1(cr), "bt601")
    for fmt in ("yuyv", "uyvy"):
        assert np.array_equal(C.to_bgr(L.packed_422(luma, cb, cr, fmt), fmt, "bt601"), want)
    nv12 = C.nv12_frame(luma, cb[:3], cr[:3])
    want = C.convert(luma, C.fancy(cb[:3]), C.fancy(cr[:3]), "jpeg")
    from tests import yuv_ref as Y
    assert np.array_equal(C.to_bgr(nv12, "nv12"), want) and np.array_equal(C.to_bgr(Y.to_nv21(nv12), "nv21"), want)
    for fmt in L.PLANAR:
        assert np.array_equal(C.to_bgr(L.planar_from_nv12(nv12, fmt), fmt), want)


# ------------------------------------------------------------------------------------------------------ names, keys, layouts
def test_colour_jpeg_is_libjpegs_integers():
    assert P.yuv_coefficients("jpeg") == JPEG == C.JPEG
    assert P.yuv_coefficients("jfif") == (0, 65536, 91881, -22553, -46802, 116130)       # "jfif" keeps its constants
    assert "jpeg" in P.COLOURS and set(P.YUV_STANDARDS) == {"jfif", "bt601", "bt709"}
    for fmt in ("nv12", "yuv420p", "uyvy", "yuv444p"):
        plan = P.ResamplePlan(HW, dict(resize=0.5), None, fmt, "jpeg")
        assert plan.yuv == JPEG and plan.key[6] == "jpeg" and plan.key != P.plan_key(HW, dict(resize=0.5), fmt, "jfif")
    assert P.ResamplePlan(HW, None, None, "rgb", "jpeg").yuv is None
    with pytest.raises(ValueError, match="p010 frames take 'bt601' or 'bt709'"):
        P.ResamplePlan(HW, None, None, "p010", "jpeg")
    with pytest.raises(ValueError, match="libjpeg"):
        P.p010_coefficients("jpeg")
    with pytest.raises(ValueError, match="colour standard 'jpg'.*jpeg"):
        P.plan_key(HW, None, "nv12", "jpg")


def test_yuv444p_shape_layout_and_key():
    assert "yuv444p" in P.ALL_FORMATS and P.SURFACE_FORMAT["yuv444p"] == 16 and P.format_code("yuv444p") == 16
    assert P.frame_shape(HW, "yuv444p") == (192, 96) and P.frame_shape((9, 17), "yuv444p") == (27, 17)       # any size
    t = P.SurfaceLayout(HW, "yuv444p")
    assert t.tight and t.key is None and (t.pitch, t.chroma_pitch, t.luma_rows, t.chroma_rows) == (96, 96, 64, 64)
    assert (t.chroma_offset, t.chroma2_offset, t.sample_end, t.image_bytes) == (64 * 96, 2 * 64 * 96, 3 * 64 * 96, 3 * 64 * 96)
    pad = P.SurfaceLayout((9, 17), "yuv444p", pitch=23, luma_rows=12, chroma_pitch=19, image_bytes=700)
    assert (pad.chroma_offset, pad.chroma2_offset, pad.sample_end) == (12 * 23, 12 * 23 + 9 * 19, 12 * 23 + 9 * 19 + 8 * 19 + 17)
    assert pad.key == (23, 12, 19, 276, 700, 447) and "chroma2_offset=447" in repr(pad)
    d = pad.describe()
    assert "yuv444p surface of 17 x 9" in d and "two planes of 9 rows of 17 bytes at pitch 19" in d and "Cr from byte 447" in d
    for kw, words in ((dict(chroma_pitch=16), "chroma rows overlap"), (dict(chroma_offset=8 * 17 + 16), "planes overlap"),
                      (dict(chroma2_offset=9 * 17 + 8 * 17 + 16), "planes overlap"), (dict(image_bytes=3 * 9 * 17 - 1), "outside image_bytes")):
        with pytest.raises(ValueError, match=words):
            P.SurfaceLayout((9, 17), "yuv444p", **kw)
    aug = dict(resize=0.5)
    assert P.plan_key(HW, aug, "yuv444p") == (64, 96, (48, 32), (0, 0, 48, 32), False, "yuv444p", "jfif")
    assert P.plan_key(HW, aug, "yuv444p", "jfif", dict(pitch=100)) == P.plan_key(HW, aug, "yuv444p") + ((100, 64, 100, 6400, 19196, 12800),)
    plan = P.ResamplePlan(HW, dict(resize=1, crop=(0, 3, 96, 8)), None, "yuv444p", "jpeg")
    assert plan.frame_shape == (192, 96) and plan.bytes_per_image(288)["source"] == 3 * 5 * 96
    assert "[..., 192, 96] yuv444p frames" in plan.layout()
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="yuv444p frames"):
        plan.run(torch.zeros(1, 96, 96, dtype=torch.uint8))


def test_chroma_enters_keys_and_descriptors_and_the_default_changes_nothing():
    aug = dict(resize=0.5)
    # the default key is today's, spelled out (tests/test_plane_ingest_host.py: test_keys has the same literals)
    old = {("bgr", None): (64, 96, (48, 32), (0, 0, 48, 32), False, "bgr", None),
           ("nv12", None): (64, 96, (48, 32), (0, 0, 48, 32), False, "nv12", "bt601"),
           ("nv12", 128): (64, 96, (48, 32), (0, 0, 48, 32), False, "nv12", "bt601", (128, 64, 128, 64 * 128, 64 * 128 + 31 * 128 + 96)),
           ("yuyv", None): (64, 96, (48, 32), (0, 0, 48, 32), False, "yuyv", "bt601")}
    for (fmt, pitch), key in old.items():
        layout = None if pitch is None else dict(pitch=pitch)
        assert P.plan_key(HW, aug, fmt, "bt601", layout) == key == P.plan_key(HW, aug, fmt, "bt601", layout, 0.0, "replicate")
        assert P.plan_key(HW, aug, fmt, "bt601", layout, chroma="replicate") == key
        if fmt != "bgr":
            assert P.plan_key(HW, aug, fmt, "bt601", layout, 0.0, "jpeg") == key + (("chroma", "jpeg"),)
            assert P.plan_key(HW, aug, fmt, "bt601", layout, 5.0, "jpeg") == key + (("roll", 5.0), ("chroma", "jpeg"))
            assert P.ResamplePlan(HW, aug, None, fmt, "bt601", layout, chroma="jpeg").key == key + (("chroma", "jpeg"),)
    import inspect
    for fn in (P.plan_key, P.ResamplePlan.__init__, P.CameraSource.__init__):
        assert list(inspect.signature(fn).parameters)[-1] == "chroma" and inspect.signature(fn).parameters["chroma"].default == "replicate"
    assert [P.format_code(f, "jpeg") for f in P.CHROMA_JPEG_FORMATS] == [0x101, 0x102, 0x108, 0x108, 0x109, 0x10A]
    assert [P.format_code(f) for f in P.CHROMA_JPEG_FORMATS] == [1, 2, 8, 8, 9, 10]
    # a rig: the default descriptors are today's bytes; chroma="jpeg" changes one camera's format code and key, and nothing else
    def rig(chroma):
        return P.RigPlan([P.CameraSource(HW, dict(resize=0.5, crop=(4, 4, 44, 28))),
                          P.CameraSource((100, 168), dict(resize=0.25, crop=(1, 1, 41, 25)), "nv12", "jpeg", dict(pitch=176), 0.0, chroma),
                          P.CameraSource(HW, dict(resize=0.5, crop=(0, 0, 40, 24)), "nv12", layout=dict(pitch=112))])
    base, same, jpeg = rig("replicate"), P.RigPlan([P.CameraSource(s.src_hw, s.aug_config, s.frame_format, s.colour, s.surface)
                                                    for s in rig("replicate").sources]), rig("jpeg")
    raw = lambda r: bytes(memoryview(r.descriptors()))   # noqa: E731
    assert raw(base) == raw(same) and base.key == same.key and [c.format for c in base.descriptors()] == [0, 1, 1]
    cams = jpeg.descriptors()
    assert [c.format for c in cams] == [0, 0x101, 1] and jpeg.key != base.key and jpeg.sources[1].key[-2] == ("chroma", "jpeg")
    cams[1].format = 1
    assert bytes(memoryview(cams)) == raw(base)
    assert "jpeg chroma" in jpeg.sources[1].describe() and "jpeg chroma" not in base.sources[1].describe()
    # the far rows count as read: rows 3 .. 7 need chroma rows 1 .. 3, and row 4 above them (odd last row 7 -> row 4)
    a = P.ResamplePlan(HW, dict(resize=1, crop=(0, 3, 96, 8)), None, "nv12").bytes_per_image(288)["source"]
    b = P.ResamplePlan(HW, dict(resize=1, crop=(0, 3, 96, 8)), None, "nv12", chroma="jpeg").bytes_per_image(288)["source"]
    assert (a, b) == (5 * 96 + 3 * 96, 5 * 96 + 4 * 96)


@pytest.mark.parametrize("fmt,words", [("p010", "10-bit"), ("bgr", "no chroma planes"), ("rgb", "no chroma planes"), ("bgra", "no chroma planes"),
                                       ("rgba", "no chroma planes"), ("yuv444p", "its own chroma sample")])
def test_chroma_is_refused_in_words(fmt, words):
    colour = "bt601" if fmt == "p010" else "jfif"
    for make in (lambda: P.ResamplePlan(HW, None, None, fmt, colour, chroma="jpeg"), lambda: P.CameraSource(HW, None, fmt, colour, chroma="jpeg"),
                 lambda: P.plan_key(HW, None, fmt, colour, chroma="jpeg")):
        with pytest.raises(ValueError, match=words) as err:
            make()
        assert "chroma='jpeg'" in str(err.value) and fmt in str(err.value)
    with pytest.raises(ValueError, match="chroma='sited'.*replicate"):
        P.ResamplePlan(HW, None, None, "nv12", chroma="sited")


# ------------------------------------------------------------------------------------------------------------------ runners
@functools.lru_cache(maxsize=None)
def _cpu_model():
    from tests.helpers import build_product_head
    head = build_product_head(dict(image_wh=(176, 64), num_anchor=48, num_temp=32, num_output=20, bs=1), "cpu")
    return types.SimpleNamespace(head=head, parameters=head.parameters)


def _runner(cls=None, **kw):
    import torch
    from simpb_amd.runner import FrameRunner
    return (cls or FrameRunner)(_cpu_model(), 1, (64, 176), capacity=128, device=torch.device("cpu"), use_graph=False, **kw)


def test_runner_takes_and_refuses_raw_chroma():
    import inspect
    from simpb_amd import runner
    assert inspect.signature(runner.FrameRunner.__init__).parameters["raw_chroma"].default is None
    src = (160, 400)
    assert _runner(raw_input=src).raw_chroma == "replicate" and _runner(raw_input=src, raw_format="nv12", raw_chroma="replicate").raw_chroma == "replicate"
    r = _runner(raw_input=src, raw_format="nv12", raw_colour="jpeg", raw_chroma="jpeg", raw_roll=2.0)
    assert (r.raw_chroma, r.raw_colour) == ("jpeg", "jpeg") and tuple(r.raw.shape[-2:]) == (240, 400)
    assert tuple(_runner(raw_input=src, raw_format="yuv444p", raw_colour="jpeg").raw.shape[-2:]) == (480, 400)
    for cls in (runner.PipelinedRunner, runner.SplitPipelinedRunner):   # (they pass FrameRunner's arguments through)
        assert issubclass(cls, runner.FrameRunner)
    with pytest.raises(ValueError, match="raw_chroma describes raw frames: it needs raw_input"):
        _runner(raw_chroma="jpeg")
    cams = _cpu_model().head.num_cams
    rig = [P.CameraSource(src, dict(resize=0.44, crop=(0, 6, 176, 70)), "nv12", chroma="jpeg")] * cams
    with pytest.raises(ValueError, match="CameraSource brings its own chroma"):
        _runner(raw_rig=rig, raw_chroma="jpeg")
    assert [c.format for c in P.RigPlan(rig).descriptors()] == [0x101] * cams
    for fmt, colour, words in (("p010", "bt601", "10-bit"), ("bgr", "jfif", "no chroma planes"), ("yuv444p", "jpeg", "its own chroma sample")):
        with pytest.raises(ValueError, match=words):
            _runner(raw_input=src, raw_format=fmt, raw_colour=colour, raw_chroma="jpeg")
    with pytest.raises(ValueError, match="p010 frames take"):
        _runner(raw_input=src, raw_format="p010", raw_colour="jpeg")
    with pytest.raises(ValueError, match="chroma='fancy'"):
        _runner(raw_input=src, raw_format="nv12", raw_chroma="fancy")


# ------------------------------------------------------------------------------------------------------------- entry points
def _planes_call(fn, out, tail=(), **changed):
    """A consistent padded nv12 batch for the planes / roll entry point, one argument changed; `out` is a real host buffer."""
    null, ok = ctypes.c_void_p(0), ctypes.c_void_p(64)
    ints = dict(num_images=2, src_height=64, src_width=96, out_height=32, out_width=48, taps_x=9, taps_y=9, src_row0=0, src_rows=64,
                flip=0, swap_rb=1, format=FLAG | 1, pitch=128, chroma_pitch=128, chroma_offset=80 * 128, chroma2_offset=0,
                image_stride=80 * 128 + 32 * 128, yoff=0, iy=65536, irv=91881, igu=-22554, igv=-46802, ibu=116130)
    vals = dict(ints, **changed)
    return fn(ctypes.c_void_p(out.ctypes.data), ok, null, ok, ok, ok, ok, ok, ok, ok, ok, *vals.values(), *tail, null)


def _out_buffer():
    raw = np.full(4096 + 16, 0xA5, np.uint8)
    at = (-raw.ctypes.data) % 16
    return raw, raw[at:at + 4096]


def test_c_entries_refuse_the_flag_where_it_means_nothing_and_leave_the_output_alone():
    """Every call is refused before any HIP call (tests/test_capi.py), so this runs without a device; the base arguments are a
    consistent batch for the code at hand, so the refusal has the one cause its line names."""
    lib = _lib.lib()
    raw, out = _out_buffer()
    six = (ctypes.c_int * 6)(65536, 0, 32768, 0, 65536, 32768)
    bgr = dict(pitch=300, chroma_pitch=0, chroma_offset=0, image_stride=64 * 300)
    p010 = dict(pitch=256, chroma_pitch=256, chroma_offset=80 * 256, image_stride=80 * 256 + 32 * 256, yoff=16)
    full = dict(pitch=128, chroma_pitch=128, chroma_offset=80 * 128, chroma2_offset=80 * 128 + 64 * 128, image_stride=80 * 128 + 128 * 128)
    cases = [dict(bgr, format=FLAG | 0), dict(bgr, format=FLAG | 11), dict(dict(bgr, pitch=400, image_stride=64 * 400), format=FLAG | 12),
             dict(dict(bgr, pitch=400, image_stride=64 * 400), format=FLAG | 13), dict(p010, format=FLAG | 3), dict(full, format=FLAG | 16),
             dict(format=0x200 | 1), dict(format=0x300 | 1), dict(format=0x1000 | 1), dict(format=(1 << 30) | 1), dict(full, format=14),
             dict(full, format=15), dict(full, format=17), dict(format=FLAG | 4), dict(format=FLAG | 14), dict(format=FLAG), dict(format=-FLAG),
             # 4:4:4 planes that overlap: Cr inside Cb, Cb inside Cr, Cb inside the luma plane, a chroma pitch below the row
             dict(full, format=16, chroma2_offset=80 * 128 + 63 * 128 + 95), dict(full, format=16, chroma2_offset=80 * 128),
             dict(full, format=16, chroma_offset=63 * 128 + 95), dict(full, format=16, chroma_pitch=95),
             dict(full, format=16, image_stride=80 * 128 + 64 * 128 + 63 * 128 + 95),
             # the flag changes no layout rule of its format
             dict(chroma_pitch=95), dict(src_width=97), dict(src_height=65, src_rows=65), dict(chroma_offset=63 * 128 + 95), dict(iy=0),
             dict(format=FLAG | 9, src_width=95, pitch=400, chroma_pitch=0, chroma_offset=0, image_stride=64 * 400),
             dict(format=FLAG | 8, chroma_pitch=64, chroma2_offset=80 * 128 + 31 * 64 + 47, image_stride=40000)]
    for kw in cases:
        assert _planes_call(lib.simpb_preprocess_planes_nhwc4_f16, out, **kw) == 1, kw
        assert _planes_call(lib.simpb_preprocess_roll_nhwc4_f16, out, (six, 1), **kw) == 1, kw
    # the surface entry point takes codes 0..3 and no flag
    null, ok = ctypes.c_void_p(0), ctypes.c_void_p(64)
    for code in (FLAG | 1, FLAG | 2, 16, 8):
        assert lib.simpb_preprocess_surface_nhwc4_f16(ctypes.c_void_p(out.ctypes.data), ok, null, ok, ok, ok, ok, ok, ok, ok, ok, 2, 64, 96, 32, 48,
                                                      9, 9, 0, 64, 0, 1, code, 128, 128, 80 * 128, 80 * 128 + 32 * 128, *JPEG, null) == 1, code
    assert (raw == 0xA5).all()


def test_rig_entries_refuse_the_flag_where_it_means_nothing():
    lib = _lib.lib()
    raw, out = _out_buffer()
    rig = P.RigPlan([P.CameraSource(HW, dict(resize=0.5, crop=(4, 4, 44, 28))),
                     P.CameraSource((100, 168), dict(resize=0.25, crop=(1, 1, 41, 25)), "nv12", "jpeg", dict(pitch=176), chroma="jpeg"),
                     P.CameraSource(HW, dict(resize=0.5, crop=(0, 0, 40, 24)), "yuv444p", "jpeg", dict(pitch=112, luma_rows=72)),
                     P.CameraSource(HW, dict(resize=0.5, crop=(0, 0, 40, 24)), "p010", "bt601")])
    assert [c.format for c in rig.descriptors()] == [0, 0x101, 16, 3]
    one = ctypes.c_void_p(64)
    lens = (sum(k.size for k in rig.kx), 4 * 40, sum(k.size for k in rig.ky), 4 * 24, rig.mid_rows)
    rolls = (ctypes.c_int * 24)(*([65536, 0, 32768, 0, 65536, 32768] * 4))

    def call(changed):
        cams = rig.descriptors()
        for (c, field), v in changed.items():
            setattr(cams[c], field, v)
        args = (ctypes.c_void_p(out.ctypes.data), one, one, one, one, one, one, one, one, one, cams, 4, 8, 24, 40, *lens, 1)
        return lib.simpb_preprocess_rig_nhwc4_f16(*args, None), lib.simpb_preprocess_rig_roll_nhwc4_f16(*args, rolls, None)

    sf = rig.surfaces[2]
    bad = [{(0, "format"): FLAG | 0}, {(3, "format"): FLAG | 3}, {(2, "format"): FLAG | 16}, {(1, "format"): 0x200 | 1}, {(1, "format"): 0x301},
           {(2, "format"): 14}, {(2, "format"): 15}, {(2, "chroma2_offset"): sf.chroma_offset + 63 * 112 + 95}, {(2, "chroma_pitch"): 95},
           {(1, "chroma_pitch"): 167}, {(1, "src_height"): 99}]
    for changed in bad:
        assert call(changed) == (1, 1), changed
    assert (raw == 0xA5).all()
