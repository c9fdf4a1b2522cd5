"""GPU: planar 4:2:0 ("yuv420p" / "yvu420p"), packed 4:2:2 ("yuyv" / "uyvy") and RGB-order frames ("rgb" / "bgra" / "rgba") through
the ingest (csrc/preprocess.hip: simpb_preprocess_planes_nhwc4_f16, and the rig entry). The statement under test: the output
equals the BGR plan's output on the host-converted frames (tests/planes_ref.py: to_bgr, the witness's integer rule with replicated
chroma, or a byte permutation), bit for bit; the BGR plan itself is pinned to Pillow by tests/test_gpu_preprocess.py. Pad bytes
are 0xFF in one run and random in another: the output may not depend on them. No test passes an address outside a live tensor."""
import ctypes

import numpy as np
import pytest
import torch

from simpb_amd import _lib
from simpb_amd import preprocess as P
from tests import planes_ref as L
from tests import yuv_ref as Y

pytestmark = pytest.mark.gpu

HALF = dict(resize=0.5)
NORM = P.IMG_NORM_CFG
FORMATS = L.NEW
_cache = {}


def same_bits(got, expected, what=""):
    got, expected = got.cpu(), expected.cpu()
    assert got.shape == expected.shape and got.dtype == expected.dtype == torch.float16, (what, got.shape, expected.shape)
    a, b = got.contiguous().view(torch.int16), expected.contiguous().view(torch.int16)
    assert torch.equal(a, b), (what, int((a != b).sum()), "elements differ")


def frames_of(fmt, hw, n=2, seed=40):
    """Random tight frames u8 [n, ...] of a format (every byte random: most YCbCr triples lie outside the gamut, alpha is noise)."""
    key = ("frames", fmt, hw, n, seed)
    if key not in _cache:
        _cache[key] = np.random.RandomState(seed).randint(0, 256, (n,) + P.frame_shape(hw, fmt)).astype(np.uint8)
    return _cache[key]


def bgr_output(bgr, aug, norm=NORM):
    """The BGR plan's output on host pictures u8 [n, Hs, Ws, 3]."""
    bgr = np.ascontiguousarray(bgr)
    out = P.ResamplePlan(bgr.shape[1:3], aug, norm).run(torch.from_numpy(bgr).cuda())
    torch.cuda.synchronize()
    return out.cpu()


def expected_of(fmt, hw, aug, norm=NORM, standard="jfif", n=2, seed=40):
    key = ("expected", fmt, hw, repr(sorted(aug.items())), norm["to_rgb"], standard, n, seed)
    if key not in _cache:
        _cache[key] = bgr_output(L.to_bgr(frames_of(fmt, hw, n, seed), fmt, standard), aug, norm)
    return _cache[key]


def own_allocations(surf, offset=0):
    """Each surface of u8 [n, image_bytes] in its own device allocation, `offset` bytes behind the allocation's first byte."""
    held = []
    for i in range(surf.shape[0]):
        buf = torch.full((surf.shape[-1] + offset,), 0xEE, dtype=torch.uint8, device="cuda")
        buf[offset:].copy_(torch.from_numpy(surf[i]))
        held.append(buf[offset:])
    return held


def run_forms(tight, hw, aug, fmt, kw, expected, norm=NORM, standard="jfif", what=""):
    """`tight` frames in surfaces of layout `kw` (None: the tight form): the contiguous batch with 0xFF and with random pad bytes
    and the address table all equal `expected`."""
    plan = P.ResamplePlan(hw, aug, norm, fmt, standard, layout=kw)
    assert plan.surface.tight == (kw is None)
    for fill in (0xFF, np.random.RandomState(99)):
        surf = L.pack(tight, plan.surface, fill)
        frames = surf.reshape((-1,) + plan.frame_shape)
        out = plan.run(torch.from_numpy(frames).cuda())
        torch.cuda.synchronize()
        assert not out[..., 3].any()
        same_bits(out, expected, (what, fmt, kw, "random pad" if fill != 0xFF else "0xFF pad"))
    held = own_allocations(surf)
    same_bits(plan.run_surfaces(held[::-1]), expected.flip(0), (what, fmt, kw, "address table"))
    torch.cuda.synchronize()
    return plan


def padded(fmt, hw):
    """A layout with a pitch that is no multiple of 16 and, for planar frames, planes at odd offsets."""
    hs, ws = hw
    if fmt in L.PLANAR:
        pitch = ws + 5
        cp = ws // 2 + 3
        first = (hs + 2) * pitch + 3
        second = first + (hs // 2) * cp + 2
        cb, cr = (first, second) if fmt == "yuv420p" else (second, first)
        assert first % 2 and pitch % 16
        return dict(pitch=pitch, luma_rows=hs + 2, chroma_pitch=cp, chroma_offset=cb, chroma2_offset=cr, image_bytes=second + (hs // 2) * cp + 100)
    pitch = ws * L.PIXEL_BYTES[fmt] + 3
    assert pitch % 16
    return dict(pitch=pitch, image_bytes=hs * pitch + 50)


def small(fmt):
    """The small source: an odd height where the format has one."""
    return (30, 50) if fmt in L.PLANAR else (31, 50)


# ------------------------------------------------------------------------------------------- 1. tight and padded, every format
@pytest.mark.parametrize("fmt", FORMATS)
def test_tight_frames(fmt):
    """64 x 96 -> 32 x 48 and the small source -> 15 x 25 in the tight form: batch of 2 and address table."""
    for hw in ((64, 96), small(fmt)):
        plan = run_forms(frames_of(fmt, hw), hw, HALF, fmt, None, expected_of(fmt, hw, HALF), what="tight")
        assert plan.out_hw == (hw[0] // 2, hw[1] // 2)


@pytest.mark.parametrize("fmt", FORMATS)
def test_padded_layouts(fmt):
    """A pitch that is no multiple of 16 (the alignment alternates from row to row), planes at odd offsets, tail padding; on the
    small source a crop that keeps rows 3 .. 7, so that most rows -- and the chroma rows under them -- are not needed."""
    run_forms(frames_of(fmt, (64, 96)), (64, 96), HALF, fmt, padded(fmt, (64, 96)), expected_of(fmt, (64, 96), HALF), what="padded")
    hw = small(fmt)
    aug = dict(resize=1, crop=(0, 3, 50, 8))
    plan = run_forms(frames_of(fmt, hw), hw, aug, fmt, padded(fmt, hw), expected_of(fmt, hw, aug), what="rows 3 .. 7")
    assert (plan.src_row0, plan.src_rows) == (3, 5)


@pytest.mark.parametrize("fmt", FORMATS)
def test_flip_and_channel_order(fmt):
    hw = small(fmt)
    aug, norm = dict(resize=0.5, flip=True), dict(NORM, to_rgb=False)
    run_forms(frames_of(fmt, hw), hw, aug, fmt, padded(fmt, hw), expected_of(fmt, hw, aug, norm), norm=norm, what="flip, to_rgb=False")


# ------------------------------------------------------------------------------------------- 2. planar against nv12 on the device
@pytest.mark.parametrize("standard", ["jfif", "bt601", "bt709"])
def test_planar_against_nv12_on_the_reinterleaved_frame(standard):
    hw = (64, 96)
    for fmt in L.PLANAR:
        planar = frames_of(fmt, hw, seed=41)
        nv12 = L.nv12_from_planar(planar, fmt)
        ref_plan = P.ResamplePlan(hw, HALF, NORM, "nv12", standard, layout=dict(pitch=112, luma_rows=72))
        ref = ref_plan.run(torch.from_numpy(L.pack(nv12, ref_plan.surface, 0xFF)).cuda()).clone()
        plan = P.ResamplePlan(hw, HALF, NORM, fmt, standard, layout=padded(fmt, hw))
        got = plan.run(torch.from_numpy(L.pack(planar, plan.surface, np.random.RandomState(98))).cuda())
        torch.cuda.synchronize()
        same_bits(got, ref, (fmt, standard))
        same_bits(got, bgr_output(Y.yuv420sp_to_bgr(nv12, standard), HALF), (fmt, standard, "witness"))
    # the planes read in the other order are another picture
    frame = torch.from_numpy(frames_of("yuv420p", hw, seed=41)).cuda()
    right, wrong = (P.ResamplePlan(hw, HALF, NORM, fmt, standard).run(frame).cpu() for fmt in L.PLANAR)
    assert not torch.equal(right, wrong)


# ------------------------------------------------------------------------------------------- 3. siblings
def test_yuyv_against_uyvy_on_byte_swapped_frames():
    hw = (31, 50)
    frame = frames_of("yuyv", hw, seed=42)
    for standard in ("jfif", "bt709"):
        a = P.ResamplePlan(hw, HALF, NORM, "yuyv", standard).run(torch.from_numpy(frame).cuda()).clone()
        b = P.ResamplePlan(hw, HALF, NORM, "uyvy", standard).run(torch.from_numpy(L.swap_422(frame)).cuda()).clone()
        c = P.ResamplePlan(hw, HALF, NORM, "uyvy", standard).run(torch.from_numpy(frame).cuda()).clone()
        torch.cuda.synchronize()
        same_bits(a, b, standard)
        assert not torch.equal(a.cpu(), c.cpu())


def test_rgb_family_against_bgr_and_alpha_is_ignored():
    hw = (31, 50)
    rng = np.random.RandomState(43)
    bgr = rng.randint(0, 256, (2,) + hw + (3,)).astype(np.uint8)
    ref = bgr_output(bgr, HALF)
    for fmt in ("rgb", "bgra", "rgba"):
        outs = []
        for alpha in (rng, 0):
            plan = P.ResamplePlan(hw, HALF, NORM, fmt, layout=padded(fmt, hw))
            out = plan.run(torch.from_numpy(L.pack(L.from_bgr(bgr, fmt, alpha), plan.surface, rng)).cuda())
            torch.cuda.synchronize()
            outs.append(out.cpu())
        same_bits(outs[0], ref, fmt)
        same_bits(outs[1], ref, fmt + ", alpha 0")
    swapped = P.ResamplePlan(hw, HALF, NORM, "rgb").run(torch.from_numpy(bgr).cuda())      # BGR bytes read as RGB: another picture
    assert not torch.equal(swapped.cpu(), ref)


# ------------------------------------------------------------------------------------------- 4. bytewise staging
@pytest.mark.parametrize("fmt", FORMATS)
def test_surfaces_one_byte_past_a_16_byte_boundary(fmt):
    """Every row of every plane starts off the 16-byte grid (pitches and plane offsets are multiples of 16, the base is not): the
    bytewise staging path alone."""
    hw = (64, 96)
    kw = dict(pitch=128 * (1 if fmt in L.PLANAR else L.PIXEL_BYTES[fmt]))
    if fmt in L.PLANAR:
        kw.update(luma_rows=66, chroma_pitch=64)
    plan = P.ResamplePlan(hw, HALF, NORM, fmt, layout=kw)
    assert plan.surface.pitch % 16 == plan.surface.chroma_offset % 16 == plan.surface.chroma2_offset % 16 == 0
    held = own_allocations(L.pack(frames_of(fmt, hw), plan.surface, np.random.RandomState(97)), offset=1)
    assert all(t.data_ptr() % 16 == 1 for t in held)
    same_bits(plan.run_surfaces(held), expected_of(fmt, hw, HALF), fmt)
    torch.cuda.synchronize()


def test_alignment_alternates_from_row_to_row_at_pitch_100():
    """Pitch 100: every fourth row starts on a 16-byte boundary (chunks and a bytewise tail), the others do not."""
    for fmt, hw, kw in (("yuv420p", (64, 96), dict(pitch=100)), ("uyvy", (31, 50), dict(pitch=100))):
        plan = P.ResamplePlan(hw, HALF, NORM, fmt, layout=kw)
        held = own_allocations(L.pack(frames_of(fmt, hw), plan.surface, 0xFF))
        assert all(t.data_ptr() % 16 == 0 for t in held)
        same_bits(plan.run_surfaces(held), expected_of(fmt, hw, HALF), fmt)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 5. the widest source
@pytest.mark.parametrize("fmt", ["bgra", "yuyv"])
def test_widest_source(fmt):
    """6 x 4096 -> 3 x 2048: the staged row of 16384 (bgra) / 8192 (yuyv) bytes, the (B, G, R) row of 12288 and the widest output."""
    hw = (6, 4096)
    plan = P.ResamplePlan(hw, HALF, NORM, fmt)
    assert plan.out_hw == (3, 2048)
    out = plan.run(torch.from_numpy(frames_of(fmt, hw, seed=44)).cuda())
    torch.cuda.synchronize()
    same_bits(out, expected_of(fmt, hw, HALF, seed=44), fmt)
    with pytest.raises(ValueError, match="outside the kernel's limits"):
        P.ResamplePlan((6, 4098), HALF, NORM, fmt).run(torch.zeros((1,) + P.frame_shape((6, 4098), fmt), dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------- 6. / 7. the entry point itself
def c_arguments(plan, n):
    """(tables, ints up to swap_rb) of a reserved plan as both surface entry points take them."""
    d = plan._dev
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    tables = [p(d["mid"]), p(d["kx"]), p(d["xlo"]), p(d["xn"]), p(d["ky"]), p(d["ylo"]), p(d["yn"]), p(d["lut"])]
    hs, ws = plan.src_hw
    h, w = plan.out_hw
    return tables, [n, hs, ws, h, w, plan.taps_x, plan.taps_y, plan.src_row0, plan.src_rows, int(plan.flip), int(plan.swap_rb)]


@pytest.mark.parametrize("fmt,standard,kw", [("bgr", "jfif", dict(pitch=300)), ("nv12", "bt601", dict(pitch=112, luma_rows=72)),
                                             ("nv21", "jfif", dict(pitch=100)), ("p010", "bt709", dict(pitch=256, luma_rows=80))])
def test_codes_0_to_3_equal_the_older_entry(fmt, standard, kw):
    hw = (64, 96)
    plan = P.ResamplePlan(hw, HALF, NORM, fmt, standard, layout=kw).reserve(2, "cuda")
    sf = plan.surface
    src = torch.from_numpy(np.random.RandomState(45).randint(0, 256, (2, sf.image_bytes)).astype(np.uint8)).cuda()
    table = torch.tensor([src[1].data_ptr(), src[0].data_ptr()], dtype=torch.int64, device="cuda")
    tables, ints = c_arguments(plan, 2)
    yuv = list(plan.yuv) if plan.yuv is not None else [0, 1, 0, 0, 0, 0]
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    null, stream = ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = P.SURFACE_FORMAT[fmt]
    for images in ((p(src), null), (null, p(table))):
        old = torch.full((2, 32, 48, 4), 7.0, dtype=torch.float16, device="cuda")
        new = torch.full((2, 32, 48, 4), 9.0, dtype=torch.float16, device="cuda")
        assert _lib.lib().simpb_preprocess_surface_nhwc4_f16(p(old), *images, *tables, *ints, code, sf.pitch, sf.chroma_pitch, sf.chroma_offset,
                                                             sf.image_bytes, *yuv, stream) == 0
        torch.cuda.synchronize()
        # (chroma2_offset is not looked at for these formats: any value is taken)
        assert _lib.lib().simpb_preprocess_planes_nhwc4_f16(p(new), *images, *tables, *ints, code, sf.pitch, sf.chroma_pitch, sf.chroma_offset,
                                                            12345, sf.image_bytes, *yuv, stream) == 0
        torch.cuda.synchronize()
        same_bits(new, old, fmt)
        assert not bool((old == 7.0).all())


def test_refused_call_leaves_the_output_untouched():
    hw, fmt = (64, 96), "yuv420p"
    plan = P.ResamplePlan(hw, HALF, NORM, fmt, layout=dict(pitch=128, luma_rows=80)).reserve(2, "cuda")
    sf = plan.surface
    src = torch.from_numpy(L.pack(frames_of(fmt, hw), sf, 0xFF)).cuda()
    out = torch.full((2, 32, 48, 4), 7.0, dtype=torch.float16, device="cuda")
    tables, ints = c_arguments(plan, 2)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    null, stream = ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = _lib.lib().simpb_preprocess_planes_nhwc4_f16
    good = [8, sf.pitch, sf.chroma_pitch, sf.chroma_offset, sf.chroma2_offset, sf.image_bytes] + list(plan.yuv)

    def changed(i, v):
        return good[:i] + [v] + good[i + 1:]

    # Cr on top of Cb, Cr inside the luma plane, a chroma pitch below the row, an image stride that ends before the last sample,
    # and the codes between the two families
    for tail in (changed(4, sf.chroma_offset), changed(4, 128), changed(2, 47), changed(5, sf.sample_end - 1), changed(0, 5), changed(0, 4),
                 changed(0, 7)):
        assert fn(p(out), p(src), null, *tables, *ints, *tail, stream) == 1, tail
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert fn(p(out), p(src), null, *tables, *ints, *good, stream) == 0     # (and the same buffers are taken when the arguments are right)
    torch.cuda.synchronize()
    same_bits(out, expected_of(fmt, hw, HALF), "the good call")


# ------------------------------------------------------------------------------------------- 8. a rig
STREAMS = 2


def rig_sources():
    return [P.CameraSource((64, 96), dict(resize=0.5, crop=(4, 4, 44, 28))),
            P.CameraSource((100, 168), dict(resize=0.25, crop=(1, 1, 41, 25)), "nv12", layout=dict(pitch=176)),
            P.CameraSource((64, 96), dict(resize=0.5, crop=(0, 0, 40, 24)), "yuv420p", "bt601", padded("yuv420p", (64, 96))),
            P.CameraSource((31, 50), dict(resize=1, crop=(5, 3, 45, 27), flip=True), "uyvy", "bt709", dict(pitch=103)),
            P.CameraSource((12, 20), dict(resize=2, crop=(0, 0, 40, 24)), "bgra")]


def rig_surfaces(rig):
    """STREAMS * 5 device tensors in (stream, camera) order, each its own allocation, random pad bytes."""
    rng = np.random.RandomState(46)
    per_cam = []
    for s in rig.sources:
        shape = (STREAMS,) + (s.src_hw + (3,) if s.frame_format == "bgr" else P.frame_shape(s.src_hw, s.frame_format))
        per_cam.append(own_allocations(L.pack(rng.randint(0, 256, shape).astype(np.uint8), s.surface, rng)))
    return [per_cam[c][s] for s in range(STREAMS) for c in range(len(per_cam))]


def test_rig_of_old_and_new_formats():
    """bgr + nv12 + yuv420p (padded) + uyvy (odd height) + bgra, two streams, one image missing: every output block is that
    camera's own plan's (which the tests above pin to the BGR plan), the skipped block is zeros."""
    rig = P.RigPlan(rig_sources())
    assert rig.out_hw == (24, 40) and [c.format for c in rig.descriptors()] == [0, 1, 8, 10, 12]
    tensors = rig_surfaces(rig)
    given = list(tensors)
    given[7] = None      # stream 1, camera 2
    out = torch.full((10, 24, 40, 4), 7.0, dtype=torch.float16, device="cuda")
    assert rig.run_surfaces(given, out=out) is out
    torch.cuda.synchronize()
    assert not out[..., 3].any()
    for c, s in enumerate(rig.sources):
        alone = s.plan().run_surfaces(tensors[c::5])
        torch.cuda.synchronize()
        if c == 2:
            same_bits(out[2], alone[0], "camera 2, stream 0")
            assert not out[7].view(torch.int16).any()
        else:
            same_bits(out[c::5], alone, ("the camera's own plan", c))
    # the new cameras against the witness as well
    for c in (2, 3, 4):
        s = rig.sources[c]
        frame = L.unpack(tensors[c].cpu().numpy()[None], s.surface)
        same_bits(out[c:c + 1], bgr_output(L.to_bgr(frame, s.frame_format, s.colour), s.aug_config), ("witness", c))


def test_rig_refuses_bad_descriptors_and_writes_nothing():
    rig = P.RigPlan(rig_sources())
    tensors = rig_surfaces(rig)
    rig.reserve(10, "cuda")
    d = rig._dev
    table = torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device="cuda")
    out = torch.full((10, 24, 40, 4), 7.0, dtype=torch.float16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    fn = _lib.lib().simpb_preprocess_rig_nhwc4_f16
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(cams):
        return fn(p(out), p(table), p(d["mid"]), *(p(d[n]) for n in rig.TABLES), p(d["lut"]), cams, 5, 10, 24, 40, d["kx"].numel(),
                  d["xlo"].numel(), d["ky"].numel(), d["ylo"].numel(), rig.mid_rows, 1, stream)

    sf = rig.surfaces[2]
    for c, field, value in ((2, "chroma2_offset", sf.chroma_offset + 5), (3, "src_width", 49), (4, "format", 6)):
        cams = rig.descriptors()
        setattr(cams[c], field, value)
        assert call(cams) == 1, (c, field)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(rig.descriptors()) == 0
    torch.cuda.synchronize()
    same_bits(out, rig.run_surfaces(tensors), "the good descriptors")
