"""GPU: a rig of cameras that differ through the ingest (csrc/preprocess.hip, simpb_preprocess_rig_nhwc4_f16): five cameras of
five sizes, all four formats, a padded and an unaligned pitch, an up-scaling, an unresampled axis and a flip, to one common
output, in two launches. Expected values come from the witnesses (tests/yuv_ref.py, surface_ref.p010_to_bgr for the picture,
preprocess_ref.nhwc4_f16 for the stem operand) and from each camera's own ResamplePlan; the path is integer arithmetic plus a
table, so every comparison is bit for bit. No test passes an address outside a live tensor."""
import ctypes

import numpy as np
import pytest
import torch

from simpb_amd import _lib
from simpb_amd import preprocess as P
from tests import preprocess_ref as R
from tests import surface_ref as S
from tests import yuv_ref as Y

pytestmark = pytest.mark.gpu

NORM = P.IMG_NORM_CFG
STREAMS = 2
P010_LAYOUT = dict(pitch=192, luma_rows=56)
_cache = {}


def noise(n, hs, ws, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, hs * 3 // 2, ws)).astype(np.uint8)


def want(bgr, aug, norm=NORM):
    return torch.from_numpy(R.nhwc4_f16(bgr, aug, norm))


def same_bits(got, expected, what=""):
    got, expected = got.cpu(), expected.cpu()
    assert got.shape == expected.shape and got.dtype == expected.dtype == torch.float16, (what, got.shape, expected.shape)
    a, b = got.contiguous().view(torch.int16), expected.contiguous().view(torch.int16)
    assert torch.equal(a, b), (what, int((a != b).sum()), "elements differ")


def sources(width=40):
    d = 40 - width
    return [P.CameraSource((64, 96), dict(resize=0.5, crop=(4, 4, 44 - d, 28))),
            P.CameraSource((100, 168), dict(resize=0.25, crop=(1, 1, 41 - d, 25)), "nv12", layout=dict(pitch=176)),
            P.CameraSource((48, 80), dict(resize=0.5, crop=(0, 0, 40 - d, 24), flip=True), "p010", "bt709", P010_LAYOUT),
            P.CameraSource((30, 50), dict(resize=1, crop=(5, 3, 45 - d, 27)), "nv21", layout=dict(pitch=54)),
            P.CameraSource((12, 20), dict(resize=2, crop=(d, 0, 40, 24)))]


def pictures(seed):
    """Per camera (surfaces u8 [STREAMS, image_bytes] with random pad bytes, the BGR pictures u8 [STREAMS, Hs, Ws, 3])."""
    if ("pictures", seed) in _cache:
        return _cache["pictures", seed]
    rng = np.random.RandomState(seed)
    srcs = sources()
    out = []
    for c, s in enumerate(srcs):
        hs, ws = s.src_hw
        if s.frame_format == "bgr":
            tight = rng.randint(0, 256, (STREAMS, hs, ws, 3)).astype(np.uint8)
            bgr = tight
        elif s.frame_format == "p010":      # all 16 bits random: true 10-bit samples with the low six bits set
            tight = rng.randint(0, 65536, (STREAMS, hs * 3 // 2, ws)).astype(np.uint16)
            tl = P.SurfaceLayout(s.src_hw, "p010")
            bgr = S.p010_to_bgr(S.pack(tight, tl), tl, s.colour)
        else:
            tight = noise(STREAMS, hs, ws, seed + 10 + c)
            bgr = Y.yuv420sp_to_bgr(tight, s.colour, 1 if s.frame_format == "nv21" else 0)
        out.append((S.pack(tight, s.surface, rng), bgr))
    _cache["pictures", seed] = out
    return out


def expected(seed, width=40):
    """f16 [STREAMS * 5, 24, width, 4] in (stream, camera) order: the witness's operand of every image."""
    if ("expected", seed, width) not in _cache:
        per_cam = [want(bgr, s.aug_config) for s, (_, bgr) in zip(sources(width), pictures(seed))]
        _cache["expected", seed, width] = torch.stack([per_cam[c][s] for s in range(STREAMS) for c in range(5)])
    return _cache["expected", seed, width]


def device_surfaces(seed, offsets=None):
    """The pictures as STREAMS * 5 device tensors in (stream, camera) order, each its own allocation; offsets[c]: bytes from the
    allocation's first byte to the surface's."""
    tensors = []
    for s in range(STREAMS):
        for c, (surf, _) in enumerate(pictures(seed)):
            off = 0 if offsets is None else offsets[c]
            buf = torch.full((surf.shape[-1] + off,), 0xEE, dtype=torch.uint8, device="cuda")
            buf[off:].copy_(torch.from_numpy(surf[s]))
            tensors.append(buf[off:])
    return tensors


def test_two_streams_ten_images():
    rig = P.RigPlan(sources())
    # what the Pillow rule gives for these cameras: different tap counts and row counts in one launch
    assert [P.coefficients(w, d)[2].shape[1] for w, d in ((96, 48), (168, 42), (80, 40), (50, 50), (20, 40))] == list(rig.taps_x) == [9, 17, 9, 1, 5]
    assert len(set(rig.src_rows)) == 5 and rig.surfaces[1].pitch == 176 and rig.surfaces[3].pitch % 16
    tensors = device_surfaces(1)
    got = rig.run_surfaces(tensors)
    torch.cuda.synchronize()
    assert got.shape == (10, 24, 40, 4) and not got[..., 3].any()
    exp = expected(1)
    for n in range(10):
        same_bits(got[n], exp[n], ("witness", n))
    for c, s in enumerate(rig.sources):
        alone = s.plan().run_surfaces(tensors[c::5])
        same_bits(got[c::5], alone, ("the camera's own plan", c))


def test_odd_output_width():
    rig = P.RigPlan(sources(38))
    assert rig.out_hw == (24, 38)
    got = rig.run_surfaces(device_surfaces(1))
    torch.cuda.synchronize()
    same_bits(got, expected(1, 38), "width 38")


def test_null_entries_are_zero_blocks():
    rig = P.RigPlan(sources())
    tensors = device_surfaces(1)
    tensors[3] = tensors[7] = None
    out = torch.full((10, 24, 40, 4), 7.0, dtype=torch.float16, device="cuda")
    assert rig.run_surfaces(tensors, out=out) is out
    torch.cuda.synchronize()
    exp = expected(1).clone()
    exp[3] = exp[7] = 0
    same_bits(out, exp, "entries 3 and 7 skipped")
    assert not out[3].view(torch.int16).any() and not out[7].view(torch.int16).any()


def test_mixed_allocation_alignment():
    rig = P.RigPlan(sources())
    tensors = device_surfaces(1, offsets=[1, 3, 2, 5, 7])
    assert [t.data_ptr() % 16 for t in tensors[:5]] == [1, 3, 2, 5, 7]
    got = rig.run_surfaces(tensors)
    torch.cuda.synchronize()
    same_bits(got, expected(1), "odd base addresses")
    odd = list(tensors)
    odd[2] = torch.zeros(tensors[2].numel() + 1, dtype=torch.uint8, device="cuda")[1:]
    with pytest.raises(ValueError, match="camera 2 of the rig.*odd address"):
        rig.run_surfaces(odd)
    with pytest.raises(ValueError, match="camera 1 of the rig.*last sample"):
        rig.run_surfaces(tensors[:1] + [tensors[1][1:]] + tensors[2:])
    with pytest.raises(ValueError, match="whole streams"):
        rig.run_surfaces(tensors[:9])


def test_captured_launch_follows_the_table():
    rig = P.RigPlan(sources()).reserve(10, "cuda")
    first, second = device_surfaces(1), device_surfaces(2, offsets=[0, 1, 0, 1, 0])
    table = torch.tensor(rig.surface_table(first)[0], dtype=torch.int64, device="cuda")
    out = torch.zeros(10, 24, 40, 4, dtype=torch.float16, device="cuda")
    rig.run_table(table, out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig.run_table(table, out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    same_bits(out, expected(1), "replay, first pictures")
    table.copy_(torch.tensor(rig.surface_table(second)[0], dtype=torch.int64))
    graph.replay()
    torch.cuda.synchronize()
    same_bits(out, expected(2), "replay, second pictures")
    assert not torch.equal(expected(1), expected(2))


def test_refused_call_leaves_the_output_untouched():
    rig = P.RigPlan(sources()).reserve(10, "cuda")
    d = rig._dev
    tensors = device_surfaces(1)
    table = torch.tensor(rig.surface_table(tensors)[0], dtype=torch.int64, device="cuda")
    out = torch.full((10, 24, 40, 4), 7.0, dtype=torch.float16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    tables = [p(d["mid"])] + [p(d[n]) for n in rig.TABLES] + [p(d["lut"])]
    lens = [d["kx"].numel(), d["xlo"].numel(), d["ky"].numel(), d["ylo"].numel(), rig.mid_rows]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = _lib.lib().simpb_preprocess_rig_nhwc4_f16

    def call(cams, num_cams=5, num_images=10):
        return fn(p(out), p(table), *tables, cams, num_cams, num_images, 24, 40, *lens, 1, stream)

    def changed(cam, **fields):
        cams = rig.descriptors()
        for k, v in fields.items():
            setattr(cams[cam], k, v)
        return cams

    wide = (_lib.RigCamera * 17)(*([rig.descriptors()[0]] * 17))
    assert call(rig.descriptors(), num_cams=0) == 1 and call(wide, num_cams=17, num_images=17) == 1
    assert call(rig.descriptors(), num_images=9) == 1                       # no whole streams
    bad = [changed(1, pitch=167),                                          # a pitch below the row's bytes
           changed(0, pitch=96 * 3 - 1),
           changed(2, pitch=191), changed(2, chroma_offset=47 * 192),    # p010: an odd pitch, planes that overlap
           changed(1, src_height=99), changed(3, src_width=49),              # odd YCbCr sizes
           changed(1, taps_x=65), changed(4, taps_y=0),  # taps above the maximum (64), none
           changed(0, src_row0=64 - rig.src_rows[0] + 1),   # rows past the source
           changed(2, mid_row=rig.mid_row[2] - 1),                           # intermediate rows inside the neighbour's
           changed(4, mid_row=rig.mid_row[4] + 1),                           # ... past the block
           changed(1, kx_offset=rig.kx_offset[1] - 1), changed(4, ky_offset=rig.ky_offset[4] + 1),
           changed(3, x_offset=rig.x_offset[2]), changed(0, format=4), changed(1, iy=0)]
    for cams in bad:
        assert call(cams) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(rig.descriptors()) == 0            # (and the same buffers are taken when the descriptors are right)
    torch.cuda.synchronize()
    same_bits(out, expected(1), "good descriptors")
