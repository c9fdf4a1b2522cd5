"""GPU: JPEG-decoder planes through the ingest (csrc/preprocess.hip: fancy_pair, SIMPB_SURFACE_CHROMA_JPEG, SIMPB_SURFACE_YUV444P).
The statement under test: the ingest's f16 [N, h, w, 4] equals, bit for bit, the host pipeline of tests/preprocess_ref.py (Pillow's
resize, crop, flip, normalise, restated) applied to the BGR picture tests/chroma_ref.py makes of the same planes -- libjpeg's
interpolated chroma, pinned to libjpeg by tests/test_chroma_host.py. Sources are the smallest at which each part can go wrong:
6 x 10 (a 3 x 5 chroma plane: every clamp, both parities), 18 x 34, and 4096 wide for the LDS bound. Pad bytes are 255 in one run and
random in another, and the planes of a padded surface sit back to back: a wrong clamp reads a neighbour's samples. No test passes
an address outside a live tensor."""
import ctypes

import numpy as np
import pytest
import torch

from simpb_amd import _lib
from simpb_amd import preprocess as P
from tests import chroma_ref as C
from tests import planes_ref as L
from tests import preprocess_ref as R
from tests import roll_ref as RR
from tests import yuv_ref as Y
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

NORM = P.IMG_NORM_CFG
FORMATS = C.INTERPOLATED + ("yuv444p",)
SOURCES = ((6, 10), (18, 34))
FLAG = 0x100
_cache = {}


def same_bits(got, expected, what=""):
    got, expected = got.cpu(), expected.cpu()
    assert got.shape == expected.shape and got.dtype == expected.dtype == torch.float16, (what, got.shape, expected.shape)
    a, b = got.contiguous().view(torch.int16), expected.contiguous().view(torch.int16)
    assert torch.equal(a, b), (what, int((a != b).sum()), "elements differ")


def frames_of(fmt, hw, n=2, seed=60):
    """Random tight frames u8 [n, ...] (every byte random: most YCbCr triples lie outside the gamut, so the clamps of the colour
    rule are at work as well)."""
    key = ("frames", fmt, hw, n, seed)
    if key not in _cache:
        _cache[key] = np.random.RandomState(seed).randint(0, 256, (n,) + P.frame_shape(hw, fmt)).astype(np.uint8)
    return _cache[key]


def host(bgr, aug, norm=NORM):
    """The host pipeline on u8 [n, Hs, Ws, 3] (B, G, R) -> f16 [n, h, w, 4]."""
    return torch.from_numpy(R.nhwc4_f16(np.ascontiguousarray(bgr), aug, norm))


def expected_of(fmt, hw, aug, norm=NORM, colour="jpeg", n=2, seed=60):
    key = ("expected", fmt, hw, repr(sorted(aug.items())), norm["to_rgb"], colour, n, seed)
    if key not in _cache:
        _cache[key] = host(C.to_bgr(frames_of(fmt, hw, n, seed), fmt, colour), aug, norm)
    return _cache[key]


def chroma_of(fmt):
    return "replicate" if fmt == "yuv444p" else "jpeg"


def own_allocations(surf, offset=0):
    """Each surface of u8 [n, image_bytes] in its own device allocation, `offset` bytes behind the allocation's first byte."""
    held = []
    for i in range(surf.shape[0]):
        buf = torch.full((surf.shape[-1] + offset,), 0xEE, dtype=torch.uint8, device="cuda")
        buf[offset:].copy_(torch.from_numpy(surf[i]))
        held.append(buf[offset:])
    return held


def run_forms(tight, hw, aug, fmt, kw, expected, norm=NORM, colour="jpeg", what="", roll=0.0):
    """The three addressing forms: the contiguous batch (pad bytes 255, then random), the address table (`run_table`) and one
    tensor per image (`run_surfaces`, off the allocation's alignment) all equal `expected`."""
    plan = P.ResamplePlan(hw, aug, norm, fmt, colour, layout=kw, roll=roll, chroma=chroma_of(fmt))
    assert plan.surface.tight == (kw is None)
    for fill in (0xFF, np.random.RandomState(98)):
        surf = C.pack(tight, plan.surface, fill)
        out = plan.run(torch.from_numpy(surf.reshape((-1,) + plan.frame_shape)).cuda())
        torch.cuda.synchronize()
        assert not out[..., 3].any()
        same_bits(out, expected, (what, fmt, kw, "random pad" if fill != 0xFF else "255 pad"))
    batch = torch.from_numpy(surf).cuda()
    table = torch.tensor([batch[i].data_ptr() for i in range(batch.shape[0])][::-1], dtype=torch.int64, device="cuda")
    same_bits(plan.run_table(table), expected.flip(0), (what, fmt, kw, "address table"))
    held = own_allocations(surf, offset=1)
    same_bits(plan.run_surfaces(held), expected, (what, fmt, kw, "raw surfaces"))
    torch.cuda.synchronize()
    return plan


def padded(fmt, hw):
    """A pitch that is no multiple of 16 and planes back to back: a plane starts at the byte after the one before it ends."""
    hs, ws = hw
    if fmt in L.PACKED_422:
        pitch = 2 * ws + 3
        assert pitch % 16
        return dict(pitch=pitch)
    pitch = ws + 3
    assert pitch % 16
    luma_end = (hs - 1) * pitch + ws
    if fmt in ("nv12", "nv21"):
        return dict(pitch=pitch, chroma_pitch=ws + 1, chroma_offset=luma_end)
    rows, cw = (hs, ws) if fmt == "yuv444p" else (hs // 2, ws // 2)
    cp = cw + 1
    first, second = luma_end, luma_end + (rows - 1) * cp + cw
    cb, cr = (second, first) if fmt == "yvu420p" else (first, second)
    return dict(pitch=pitch, chroma_pitch=cp, chroma_offset=cb, chroma2_offset=cr)


# ------------------------------------------------------------------------------------ 1. every format, tight and padded, three forms
@pytest.mark.parametrize("fmt", FORMATS)
def test_whole_picture_at_identity_and_half_size(fmt):
    """The whole source (every clamp of the upsampler: first and last column, first and last row, both parities) at identity
    size, where the ingest's output is the converted picture itself through the table, and resized to half."""
    for hw in SOURCES:
        for aug in (dict(resize=1), dict(resize=0.5)):
            run_forms(frames_of(fmt, hw), hw, aug, fmt, None, expected_of(fmt, hw, aug), what="tight")
            run_forms(frames_of(fmt, hw), hw, aug, fmt, padded(fmt, hw), expected_of(fmt, hw, aug), what="padded")


@pytest.mark.parametrize("fmt", FORMATS)
def test_middle_rows_flipped(fmt):
    """A crop that keeps the middle rows only (18 x 34: rows 6 .. 9; 6 x 10: rows 2 .. 3): the far chroma row of the first needed
    row lies above the needed range and that of the last below it. Flipped, BGR channel order, padded."""
    norm = dict(NORM, to_rgb=False)
    for hw, rows in (((18, 34), (6, 10)), ((6, 10), (2, 4)), ((18, 34), (7, 9))):
        aug = dict(resize=1, crop=(3, rows[0], hw[1] - 2, rows[1]), flip=True)
        plan = run_forms(frames_of(fmt, hw), hw, aug, fmt, padded(fmt, hw), expected_of(fmt, hw, aug, norm), norm=norm, what="middle rows")
        assert (plan.src_row0, plan.src_rows) == (rows[0], rows[1] - rows[0])


def test_colour_standards_and_the_replicated_default():
    """The interpolated samples go through whatever colour the plan names; chroma="replicate" is still the replicated picture."""
    hw, aug = (18, 34), dict(resize=0.5)
    for colour in ("jfif", "bt601", "bt709"):
        run_forms(frames_of("nv12", hw), hw, aug, "nv12", padded("nv12", hw), expected_of("nv12", hw, aug, colour=colour), colour=colour)
    frames = frames_of("nv12", hw)
    out = P.ResamplePlan(hw, aug, NORM, "nv12", "jfif").run(torch.from_numpy(frames).cuda())
    same_bits(out, host(Y.yuv420sp_to_bgr(frames, "jfif"), aug), "replicated")
    assert not torch.equal(out.cpu(), expected_of("nv12", hw, aug, colour="jfif"))


# ------------------------------------------------------------------------------------------------------- 2. the LDS bound
@pytest.mark.parametrize("fmt", ["nv12", "yvu420p", "uyvy", "yuv444p"])
def test_width_4096(fmt):
    """The widest source the kernel takes: three staged rows of 4096 bytes (planar: halves; 4:4:4: two planes' worth) beside the
    12 KB (B, G, R) row."""
    hw, aug = (4, 4096), dict(resize=0.5)
    tight = frames_of(fmt, hw, n=1, seed=61)
    plan = P.ResamplePlan(hw, aug, NORM, fmt, "jpeg", chroma=chroma_of(fmt))
    out = plan.run(torch.from_numpy(tight).cuda())
    torch.cuda.synchronize()
    same_bits(out, expected_of(fmt, hw, aug, n=1, seed=61), (fmt, 4096))
    with pytest.raises(ValueError, match="4096"):
        P.ResamplePlan((4, 4098), aug, NORM, fmt, "jpeg", chroma=chroma_of(fmt)).upload("cuda")


# ------------------------------------------------------------------------------------------------------------- 3. a rig
def test_rig_mixes_interpolated_replicated_bgr_and_a_skipped_image():
    """One launch: an NV12 camera with jpeg chroma, an NV12 camera with replicated chroma, a BGR camera, an interpolated planar
    camera -- and one image skipped (address 0: zeros)."""
    srcs = [P.CameraSource((18, 34), dict(resize=1, crop=(2, 1, 22, 13)), "nv12", "jpeg", padded("nv12", (18, 34)), chroma="jpeg"),
            P.CameraSource((18, 34), dict(resize=1, crop=(2, 1, 22, 13)), "nv12", "jpeg", padded("nv12", (18, 34))),
            P.CameraSource((24, 40), dict(resize=0.5, crop=(0, 0, 20, 12), flip=True)),
            P.CameraSource((30, 50), dict(resize=0.5, crop=(5, 3, 25, 15)), "yvu420p", "bt601", padded("yvu420p", (30, 50)), chroma="jpeg")]
    rig = P.RigPlan(srcs)
    assert [c.format for c in rig.descriptors()] == [FLAG | 1, 1, 0, FLAG | 8]
    streams, rng = 2, np.random.RandomState(62)
    tensors, want = [], []
    for s in range(streams):
        for c, src in enumerate(srcs):
            fmt = src.frame_format
            tight = frames_of(fmt, src.src_hw, n=streams, seed=63 + (c if c > 1 else 0))[s:s + 1]   # (cameras 0 and 1: the same planes)
            if fmt == "bgr":
                bgr = tight
            elif src.chroma == "jpeg":
                bgr = C.to_bgr(tight, fmt, src.colour)
            else:
                bgr = C.convert(*[np.repeat(np.repeat(v, 2, -2), 2, -1) if i else v for i, v in enumerate(C.samples(tight, fmt))], src.colour)
            want.append(host(bgr, src.aug_config))
            surf = C.pack(tight, src.surface, rng) if fmt != "bgr" else tight.reshape(1, -1)
            tensors.append(own_allocations(surf.reshape(1, -1), offset=c % 2)[0])
    skipped = 1 * len(srcs) + 0           # stream 1, camera 0
    tensors[skipped] = None
    want[skipped] = torch.zeros_like(want[skipped])
    out = rig.run_surfaces(tensors)
    torch.cuda.synchronize()
    for i, w in enumerate(want):
        same_bits(out[i:i + 1], w, ("rig image", i))
    # the interpolated camera is not the replicated one
    assert not torch.equal(out[0], out[1])


# ----------------------------------------------------------------------------------------------------- 4. a rolled camera
def test_rolled_camera_with_jpeg_chroma():
    hw, aug, roll = (18, 34), dict(resize=1, crop=(1, 2, 31, 16)), 7.5
    tight = frames_of("nv12", hw)
    level = np.stack([R.img_transform(b, aug) for b in C.to_bgr(tight, "nv12", "jpeg")])
    rolled = np.stack([RR.rotate(img, roll) for img in level])
    want = host(rolled, dict(resize=1))
    assert (rolled != level).any()
    run_forms(tight, hw, aug, "nv12", padded("nv12", hw), want, what="rolled", roll=roll)
    run_forms(tight, hw, aug, "nv12", None, want, what="rolled, tight", roll=roll)


# -------------------------------------------------------------------------------------------------- 5. the fixture, end to end
def test_native_planes_of_a_jpeg_equal_pillows_decode():
    """The native planes of Pillow's JPEG files, packed as NV12 (4:2:0 files, chroma="jpeg") and as yuv444p (4:4:4 files), at
    identity size with colour "jpeg": Pillow's own RGB decode of the same file through the same normalisation table."""
    g = load_golden("jpeg_chroma.npz")
    for sub, fmt in ((2, "nv12"), (0, "yuv444p")):
        for h, w in ((2, 2), (6, 10), (18, 34), (32, 48)):
            name = f"s{sub}_{h}x{w}"
            y, cb, cr, rgb = (g[f"{name}_{k}"] for k in ("y", "cb", "cr", "rgb"))
            frame = (C.nv12_frame(y, cb, cr) if sub == 2 else C.frame444(y, cb, cr))[None]
            want = host(rgb[None, ..., ::-1], dict(resize=1))
            out = P.ResamplePlan((h, w), dict(resize=1), NORM, fmt, "jpeg", chroma=chroma_of(fmt)).run(torch.from_numpy(frame).cuda())
            torch.cuda.synchronize()
            same_bits(out, want, name)
            if (h, w) == (32, 48):       # colour "jfif" is not libjpeg's table: one G byte of this picture differs
                other = P.ResamplePlan((h, w), dict(resize=1), NORM, fmt, "jfif", chroma=chroma_of(fmt)).run(torch.from_numpy(frame).cuda())
                assert not torch.equal(other.cpu(), want)


# ---------------------------------------------------------------------------------------------------------- 6. refusals
def test_refused_calls_leave_the_output_untouched():
    hw, aug = (18, 34), dict(resize=0.5)
    plan = P.ResamplePlan(hw, aug, NORM, "nv12", "jpeg", layout=padded("nv12", hw), chroma="jpeg").reserve(2, "cuda")
    sf, d = plan.surface, plan._dev
    src = torch.from_numpy(C.pack(frames_of("nv12", hw), sf, 0xFF)).cuda()
    out = torch.full((2, 9, 17, 4), 7.0, dtype=torch.float16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    null, stream = ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tables = [p(d[k]) for k in ("mid", "kx", "xlo", "xn", "ky", "ylo", "yn", "lut")]
    ints = [2, *hw, *plan.out_hw, plan.taps_x, plan.taps_y, plan.src_row0, plan.src_rows, 0, 1]
    good = [FLAG | 1, sf.pitch, sf.chroma_pitch, sf.chroma_offset, 0, sf.image_bytes] + list(plan.yuv)
    lib = _lib.lib()
    six = (ctypes.c_int * 6)(*P.ROLL_IDENTITY)
    changed = lambda i, v: good[:i] + [v] + good[i + 1:]   # noqa: E731
    # the flag on BGR, P010 and 4:4:4, another high bit, the codes that are no format, and a layout the flag does not excuse
    for tail in (changed(0, FLAG | 0), changed(0, FLAG | 3), changed(0, FLAG | 16), changed(0, 0x200 | 1), changed(0, 14), changed(0, 15),
                 changed(0, FLAG | 11), changed(2, 33), changed(3, sf.chroma_offset - 1), changed(5, sf.sample_end - 1)):
        assert lib.simpb_preprocess_planes_nhwc4_f16(p(out), p(src), null, *tables, *ints, *tail, stream) == 1, tail
        assert lib.simpb_preprocess_roll_nhwc4_f16(p(out), p(src), null, *tables, *ints, *tail, six, 1, stream) == 1, tail
    assert lib.simpb_preprocess_surface_nhwc4_f16(p(out), p(src), null, *tables, *ints, *good[:4], *good[5:], stream) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    for fmt in ("p010", "bgr", "rgba", "yuv444p"):
        with pytest.raises(ValueError, match="chroma='jpeg'"):
            P.ResamplePlan(hw, aug, NORM, fmt, "bt601", chroma="jpeg")
    # (and the same buffers are taken when the arguments are right: the rolled entry point with the identity is the level picture)
    assert lib.simpb_preprocess_roll_nhwc4_f16(p(out), p(src), null, *tables, *ints, *good, six, 1, stream) == 0
    torch.cuda.synchronize()
    same_bits(out, expected_of("nv12", hw, aug), "the good call")


# ------------------------------------------------------------------------------------------------------------ 7. a runner
def test_runner_on_jpeg_planes_equals_the_runner_fed_the_decoded_pictures():
    """Two frames (the cold one and the eager warm one) on the small configuration of tests/test_gpu_plane_runner.py: a runner
    with raw_format="nv12", raw_chroma="jpeg", raw_colour="jpeg" against the same runner fed, as BGR, the picture chroma_ref makes
    of those planes. The backbone sees identical f16 operands: 3D, 2D and track ids are equal bit for bit."""
    from tests.test_gpu_plane_runner import HW, R50, _compare, _drive, _runner, pictures
    frames = 2
    nv12 = [pictures("nv12", f)[0] for f in range(frames)]
    held = [torch.from_numpy(C.to_bgr(t.numpy(), "nv12", "jpeg")) for t in nv12]
    base = _runner("FrameRunner", raw_input=HW)
    a = _drive(base, lambda f: held[f].cuda(), frames)
    r = _runner("FrameRunner", raw_input=HW, raw_format="nv12", raw_chroma="jpeg", raw_colour="jpeg")
    assert r.img is None and tuple(r.raw.shape) == (1, 6) + P.frame_shape(HW, "nv12")
    b = _drive(r, lambda f: nv12[f].cuda(), frames)
    assert r.stats == base.stats, (r.stats, base.stats)
    assert r.plan.key == P.plan_key(HW, R50, "nv12", "jpeg", chroma="jpeg") and r.plan.chroma == "jpeg"
    _compare(a, b, "nv12, jpeg chroma")
    assert not np.array_equal(held[0].numpy(), pictures("nv12", 0)[1].numpy())      # (the replicated picture is another one)
