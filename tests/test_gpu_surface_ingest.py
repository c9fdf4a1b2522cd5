"""GPU: decoder surfaces through the ingest (csrc/preprocess.hip, simpb_preprocess_surface_nhwc4_f16): padded pitch, aligned plane
height, the chroma plane at its own pitch and offset, tail padding, P010, and one allocation per image behind a pointer table.
Expected values come from the witnesses, not from the code under test: tests/yuv_ref.py (surface_ref.p010_to_bgr for 10-bit
samples) gives the BGR picture, preprocess_ref.nhwc4_f16 the stem operand; the path is integer arithmetic plus a table, so every
comparison is bit for bit. Pad bytes are 0xFF in one run and random in another: the output may not depend on them. The runners'
raw_layout= and raw_surfaces= are compared with the same runner class fed tight NV12 tensors. No test passes an address outside
a live tensor, and none frees a surface before its results are back."""
import ctypes

import numpy as np
import pytest
import torch

from simpb_amd import preprocess as P
from simpb_amd import synth
from tests import preprocess_ref as R
from tests import surface_ref as S
from tests import yuv_ref as Y

pytestmark = pytest.mark.gpu

R50 = dict(resize=0.44, crop=(0, 140, 704, 396))
HALF = dict(resize=0.5)
NORM = P.IMG_NORM_CFG
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


def run_padded(tight, hw, aug, fmt, kw, expected, norm=NORM, standard="jfif", what=""):
    """`tight` frames packed into surfaces of layout `kw`, once with 0xFF and once with random pad bytes, as a contiguous batch
    through the surface entry: both outputs equal `expected`. Returns the plan and the 0xFF surfaces (host)."""
    plan = P.ResamplePlan(hw, aug, norm, fmt, standard, layout=kw)
    assert not plan.surface.tight
    first = None
    for fill in (0xFF, np.random.RandomState(99)):
        surf = S.pack(tight, plan.surface, fill)
        first = surf if first is None else first
        out = plan.run(torch.from_numpy(surf).cuda())
        torch.cuda.synchronize()
        assert not out[..., 3].any()
        same_bits(out, expected, (what, kw, "random pad" if fill != 0xFF else "0xFF pad"))
    return plan, first


# --------------------------------------------------------------------------------------------------------------- NV12 layouts
BASE_LAYOUTS = [dict(pitch=96), dict(pitch=128), dict(pitch=100), dict(luma_rows=80),
                dict(pitch=128, luma_rows=80, chroma_pitch=112, chroma_offset=80 * 128 + 4), dict(image_bytes=96 * 96 + 1000)]


def base_case():
    """(NV12 noise u8 [3, 96, 96] of 64 x 96 pictures, the expected operand of resize 0.5 -> 32 x 48)."""
    if "base" not in _cache:
        frames = noise(3, 64, 96, 21)
        _cache["base"] = (frames, want(Y.yuv420sp_to_bgr(frames), HALF))
    return _cache["base"]


@pytest.mark.parametrize("kw", BASE_LAYOUTS, ids=["tight", "pitch128", "pitch100", "rows80", "own-chroma-plane", "tail1000"])
def test_nv12_layouts(kw):
    """64 x 96 -> 32 x 48, N = 3. pitch 96 is the tight form through the new entry point: it must equal the existing entry's
    output. With pitch 100 the 16-byte alignment alternates from row to row; chroma_offset 80 * 128 + 4 puts every chroma row
    off the 16-byte grid while the luma rows are on it."""
    frames, expected = base_case()
    run_padded(frames, (64, 96), HALF, "nv12", kw, expected)
    if kw == dict(pitch=96):
        old = P.ResamplePlan((64, 96), HALF, NORM, "nv12").run(torch.from_numpy(frames).cuda())
        same_bits(old, expected, "existing entry point")


@pytest.mark.parametrize("fmt,hw,kw", [("nv12", (30, 50), dict(pitch=64)), ("nv12", (30, 50), dict(pitch=54)),
                                       ("bgr", (30, 50), dict(pitch=160)), ("bgr", (30, 50), dict(pitch=151)),
                                       ("p010", (30, 50), dict(pitch=128)), ("p010", (30, 50), dict(pitch=102))])
def test_row_bytes_no_multiple_of_16(fmt, hw, kw):
    """50 (nv12), 150 (bgr) and 100 (p010) sample bytes per row: three, nine and six 16-byte chunks and a bytewise tail on the
    rows that start aligned, bytes alone on the others; the pad bytes right behind a row's last sample are never read."""
    hs, ws = hw
    rng = np.random.RandomState(22)
    if fmt == "bgr":
        tight = rng.randint(0, 256, (3, hs, ws, 3)).astype(np.uint8)
        expected, standard = want(tight, HALF), "jfif"
    elif fmt == "nv12":
        tight = noise(3, hs, ws, 23)
        expected, standard = want(Y.yuv420sp_to_bgr(tight), HALF), "jfif"
    else:
        tight = rng.randint(0, 65536, (3, hs * 3 // 2, ws)).astype(np.uint16)
        standard = "bt709"
        tl = P.SurfaceLayout(hw, "p010")
        expected = want(S.p010_to_bgr(S.pack(tight, tl), tl, standard), HALF)
    plan, _ = run_padded(tight, hw, HALF, fmt, kw, expected, standard=standard, what=fmt)
    assert plan.out_hw == (15, 25)


def test_chroma_row_pairing_under_a_padded_chroma_pitch():
    """Crop (0, 3, 96, 8) at resize 1: needed luma rows 3 .. 7, chroma rows 1 .. 3 at their own stride; the first needed row is
    the second half of its pair, the last the first half of its own."""
    aug = dict(resize=1, crop=(0, 3, 96, 8))
    frames = noise(2, 64, 96, 24)
    plan, _ = run_padded(frames, (64, 96), aug, "nv12", dict(pitch=128, luma_rows=80), want(Y.yuv420sp_to_bgr(frames), aug))
    assert (plan.src_row0, plan.src_rows) == (3, 5)


def test_nv21_against_nv12_on_a_padded_layout():
    frames, expected = base_case()
    kw = dict(pitch=112, luma_rows=72)
    run_padded(Y.to_nv21(frames), (64, 96), HALF, "nv21", kw, expected)
    plan = P.ResamplePlan((64, 96), HALF, NORM, "nv21", layout=kw)
    wrong = plan.run(torch.from_numpy(S.pack(frames, plan.surface, 0)).cuda())     # NV12 bytes read as NV21: another picture
    assert not torch.equal(wrong.cpu(), expected)


@pytest.mark.parametrize("aug,norm", [(dict(resize=0.5, flip=True), NORM), (HALF, dict(NORM, to_rgb=False))], ids=["flip", "bgr-order"])
def test_flip_and_channel_order_on_a_padded_layout(aug, norm):
    frames = base_case()[0]
    run_padded(frames, (64, 96), aug, "nv12", dict(pitch=128, luma_rows=80), want(Y.yuv420sp_to_bgr(frames), aug, norm), norm=norm)


# --------------------------------------------------------------------------------------------------------------------- P010
@pytest.mark.parametrize("standard", ["bt601", "bt709"])
def test_p010_lifted_frames_give_the_nv12_route(standard):
    """8-bit samples stored as v << 8 with random low bits: the NV12 witness's picture, and the NV12 route's output on the
    device, tight and padded."""
    frames = base_case()[0]
    expected = want(Y.yuv420sp_to_bgr(frames, standard), HALF)
    lifted = S.to_p010(frames, np.random.RandomState(25))
    tight = P.ResamplePlan((64, 96), HALF, NORM, "p010", standard)
    assert tight.surface.tight and tight.frame_shape == (96, 192)
    got = tight.run(torch.from_numpy(lifted.astype("<u2").view(np.uint8)).cuda())
    same_bits(got, expected, "tight")
    same_bits(got, P.ResamplePlan((64, 96), HALF, NORM, "nv12", standard).run(torch.from_numpy(frames).cuda()), "nv12 route")
    run_padded(lifted, (64, 96), HALF, "p010", dict(pitch=256, luma_rows=80), expected, standard=standard)


@pytest.mark.parametrize("kw", [dict(pitch=192), dict(pitch=224, luma_rows=72, chroma_pitch=208, chroma_offset=72 * 224 + 6)], ids=["tight", "padded"])
def test_p010_ten_bit_noise(kw):
    """All 16 bits random: true 10-bit samples, most triples outside the gamut, the low six bits set."""
    words = np.random.RandomState(26).randint(0, 65536, (3, 96, 96)).astype(np.uint16)
    tl = P.SurfaceLayout((64, 96), "p010")
    bgr = S.p010_to_bgr(S.pack(words, tl), tl, "bt709")
    assert (bgr == 0).mean() > 0.05 and (bgr == 255).mean() > 0.05      # the clamps act at both ends
    run_padded(words, (64, 96), HALF, "p010", kw, want(bgr, HALF), standard="bt709")


# ------------------------------------------------------------------------------------------------------------ pointer table
@pytest.mark.parametrize("fmt", ["nv12", "p010", "bgr"])
def test_pointer_table_equals_the_contiguous_form(fmt):
    """Three images in three allocations made in another order than they are given; image 1 starts one byte (p010: two) into
    its tensor. Equal to the contiguous batch of the same surfaces, which the tests above pin to the witness."""
    hw = (64, 96)
    rng = np.random.RandomState(27)
    if fmt == "bgr":
        tight, kw, standard = rng.randint(0, 256, (3, 64, 96, 3)).astype(np.uint8), dict(pitch=300), "jfif"
    elif fmt == "nv12":
        tight, kw, standard = noise(3, 64, 96, 28), dict(pitch=128, luma_rows=80), "jfif"
    else:
        tight, kw, standard = rng.randint(0, 65536, (3, 96, 96)).astype(np.uint16), dict(pitch=256, luma_rows=80), "bt601"
    plan = P.ResamplePlan(hw, HALF, NORM, fmt, standard, layout=kw)
    surf = torch.from_numpy(S.pack(tight, plan.surface, rng))
    batch = plan.run(surf.cuda()).clone()
    shift = 2 if fmt == "p010" else 1
    n = plan.surface.image_bytes
    held = {}
    for i in (2, 0, 1):       # allocation order
        off = shift if i == 1 else 0
        buf = torch.full((n + off,), 0xEE, dtype=torch.uint8, device="cuda")
        buf[off:].copy_(surf[i])
        held[i] = buf[off:]
    assert held[1].data_ptr() % 16 == shift
    # exactly the bytes up to the last sample suffice: a surface may end there
    short = torch.empty(plan.surface.sample_end, dtype=torch.uint8, device="cuda")
    short.copy_(surf[0][:plan.surface.sample_end])
    got = plan.run_surfaces([held[0], held[1], held[2]])
    torch.cuda.synchronize()
    same_bits(got, batch, fmt)
    same_bits(plan.run_surfaces([short, held[2], held[1]]), batch[[0, 2, 1]], fmt + " reordered")
    with pytest.raises(ValueError, match="last sample"):
        plan.run_surfaces([held[0], short[1:], held[2]])
    with pytest.raises(ValueError, match="strided view"):      # every second byte of a buffer is no surface
        plan.run_surfaces([held[0], torch.zeros(2 * n, dtype=torch.uint8, device="cuda")[::2], held[2]])
    if fmt == "p010":
        odd = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="odd address"):
            plan.run_surfaces([held[0], odd[1:], held[2]])


# ------------------------------------------------------------------------------------------------------------ full size, once
def test_full_size_padded_and_pointer_table_equal_the_tight_entry():
    """1600 x 900 as a decoder allocates it (pitch 1792, 912 luma rows), R50 plan, 6 images, both modes, against the existing
    NV12 entry point on the tight frames (which test_gpu_yuv_ingest pins to the witness)."""
    frames = noise(6, 900, 1600, 29)
    tight = P.ResamplePlan((900, 1600), R50, frame_format="nv12").run(torch.from_numpy(frames).cuda()).clone()
    plan = P.ResamplePlan((900, 1600), R50, frame_format="nv12", layout=dict(pitch=1792, luma_rows=912))
    assert plan.surface.image_bytes == 1792 * 912 + 449 * 1792 + 1600
    surf = torch.from_numpy(S.pack(frames, plan.surface, np.random.RandomState(30))).cuda()
    same_bits(plan.run(surf), tight, "contiguous")
    singles = [surf[i].clone() for i in (5, 3, 1, 0, 2, 4)]
    order = {5: 0, 3: 1, 1: 2, 0: 3, 2: 4, 4: 5}
    same_bits(plan.run_surfaces([singles[order[i]] for i in range(6)]), tight, "pointer table")
    torch.cuda.synchronize()


def test_refused_call_leaves_the_output_untouched():
    from simpb_amd import _lib
    frames, expected = base_case()
    plan = P.ResamplePlan((64, 96), HALF, NORM, "nv12", layout=dict(pitch=128, luma_rows=80)).reserve(3, "cuda")
    sf, d = plan.surface, plan._dev
    src = torch.from_numpy(S.pack(frames, sf, 0xFF)).cuda()
    table = torch.tensor([src[i].data_ptr() for i in range(3)], dtype=torch.int64, device="cuda")
    out = torch.full((3, 32, 48, 4), 7.0, dtype=torch.float16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    null = ctypes.c_void_p(0)
    tables = [p(d["mid"]), p(d["kx"]), p(d["xlo"]), p(d["xn"]), p(d["ky"]), p(d["ylo"]), p(d["yn"]), p(d["lut"])]
    good = [3, 64, 96, 32, 48, plan.taps_x, plan.taps_y, plan.src_row0, plan.src_rows, 0, 1, 1, sf.pitch, sf.chroma_pitch, sf.chroma_offset,
            sf.image_bytes] + list(plan.yuv)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = _lib.lib().simpb_preprocess_surface_nhwc4_f16

    def changed(i, v):
        return good[:i] + [v] + good[i + 1:]

    # both forms of the images, neither, a pitch below the row, an unknown format, overlapping planes, an image stride that
    # ends before the last sample, no images
    assert fn(p(out), p(src), p(table), *tables, *good, stream) == 1
    assert fn(p(out), null, null, *tables, *good, stream) == 1
    for ints in (changed(12, 95), changed(11, 4), changed(14, 63 * 128), changed(15, sf.sample_end - 1), changed(0, 0)):
        assert fn(p(out), p(src), null, *tables, *ints, stream) == 1, ints
    # an odd pitch for p010 as the only fault: 192 sample bytes per row, luma rows 257 apart (they end at byte 63 * 257 + 192),
    # chroma rows 256 apart from byte 80 * 256, images 28672 apart in a buffer that holds them; pitch 256 is taken below
    src10 = torch.zeros(3, 28672, dtype=torch.uint8, device="cuda")
    good10 = good[:11] + [3, 256, 256, 80 * 256, 28672] + good[16:]
    assert 80 * 256 + 31 * 256 + 192 <= 28672 and 63 * 257 + 192 <= 80 * 256
    assert fn(p(out), p(src10), null, *tables, *(good10[:12] + [257] + good10[13:]), stream) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert fn(p(out), p(src), null, *tables, *good, stream) == 0     # (and the same buffers are taken when the arguments are right)
    torch.cuda.synchronize()
    same_bits(out, expected, "contiguous")
    out.fill_(7.0)
    assert fn(p(out), null, p(table), *tables, *good, stream) == 0
    torch.cuda.synchronize()
    same_bits(out, expected, "table")
    assert fn(p(out), p(src10), null, *tables, *good10, stream) == 0     # (the p010 arguments with the even pitch)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- runners
PADDED = dict(pitch=1792, luma_rows=912)


def _model():
    from simpb_amd import configs, plugin
    cfg = configs.simpb_plus(anchor=synth.anchors(900))
    model = plugin.build_detector(cfg["model"]).eval()
    synth.load_procedural(model)
    model.cuda()
    model.fuse_conv_bn()
    model.half_backbone()
    return model


def _pictures():
    """Three six-camera NV12 frames u8 [1, 6, 1350, 1600] of the synthetic generator (the streams cycle over them), tight and
    packed into PADDED surfaces u8 [1, 6, image_bytes] with random pad bytes."""
    if "pictures" not in _cache:
        layout = P.SurfaceLayout((900, 1600), "nv12", **PADDED)
        tight = [Y.bgr_to_nv12(synth.raw_frames(1, f, src_hw=(900, 1600), num_cams=6)[0].numpy())[None] for f in range(3)]
        rng = np.random.RandomState(31)
        _cache["pictures"] = ([torch.from_numpy(x) for x in tight], [torch.from_numpy(S.pack(x, layout, rng)) for x in tight], layout)
    return _cache["pictures"]


def _drive(r, feed, frames, bs=1, **step_kw):
    """`frames` steps of runner r; feed(f) gives the step's img. Returns per frame (results, rec3d, rec2d)."""
    got = []
    keep = lambda res: got.append((res, r.last_rec3d.clone(), r.last_rec2d.clone()))   # noqa: E731
    for f in range(frames):
        kw = {k: v[f] for k, v in step_kw.items()}
        res = r.step(feed(f), synth.frame_metas(bs, f), **kw)
        if res is not None:
            keep(res)
    if hasattr(r, "flush"):
        keep(r.flush())
    assert len(got) == frames
    return got


def _compare(a, b, name, streams=None):
    for f, ((ra, a3, a2), (rb, b3, b2)) in enumerate(zip(a, b)):
        rows = range(a3.shape[0]) if streams is None else [i for i in range(a3.shape[0]) if streams[f][i]]
        for i in rows:
            assert torch.equal(a3[i], b3[i]), (name, f, i, "rec3d")
            assert torch.equal(a2[i], b2[i]), (name, f, i, "rec2d")
        for i, (sa, sb) in enumerate(zip(ra, rb)):
            assert (sa is None) == (sb is None), (name, f, i)
            if sa is None:
                continue
            xa, xb = sa["img_bbox"], sb["img_bbox"]
            assert xa.keys() == xb.keys(), (name, f)
            for k in xa:
                x, y = xa[k], xb[k]
                if torch.is_tensor(x) or isinstance(x, np.ndarray):
                    x, y = torch.as_tensor(x), torch.as_tensor(y)
                    assert x.shape == y.shape and torch.equal(x, y), (name, f, i, k)
                else:
                    assert np.array_equal(np.asarray(x), np.asarray(y)), (name, f, i, k)


def _runner(name, bs=1, **kw):
    from simpb_amd import runner
    return getattr(runner, name)(_model(), bs, (256, 704), capacity=1536, device=torch.device("cuda"), use_graph=True,
                                 raw_input=(900, 1600), raw_format="nv12", independent_streams=bs > 1, **kw)


class Pools:
    """Decoder surface pools: every frame's surfaces are separate device tensors out of pool f % 2, and each pool's memory is
    rewritten when it comes round again -- a replay that read a stale table would decode another frame's picture. Every tensor
    ever handed out stays referenced here until the test ends."""

    def __init__(self, padded, cams=6):
        n = padded[0].shape[-1]
        self.padded = padded
        self.pools = [[torch.zeros(n + 16, dtype=torch.uint8, device="cuda") for _ in range(cams)] for _ in range(2)]
        self.handed = []

    def frame(self, f, stream=0):
        pool = self.pools[f % 2]
        torch.cuda.synchronize()      # (the frame that read this pool two steps ago has been returned: see the lifetime rule)
        row = []
        for c, buf in enumerate(pool):
            view = buf[c % 2:c % 2 + self.padded[0].shape[-1]]     # odd cameras one byte off the allocation's alignment
            view.copy_(self.padded[(f + stream) % 3][0, c])
            row.append(view)
        self.handed.append(row)
        return row


@pytest.mark.parametrize("name,frames", [("FrameRunner", 5), ("PipelinedRunner", 8), ("SplitPipelinedRunner", 8)])
def test_runner_padded_and_pointer_forms_equal_the_tight_tensor(name, frames):
    """The backbone sees identical f16 operands in all three forms, so device records and detections are equal bit for bit over
    the cold frame, eager warm frames and replayed graphs. raw_layout: padded NV12 in one tensor. raw_surfaces: the same
    surfaces as one tensor per camera out of two alternating pools. A pipelined runner has two frames in flight, so a pool
    that comes round again belongs to a frame already returned."""
    tight, padded, layout = _pictures()
    base = _runner(name)
    a = _drive(base, lambda f: tight[f % 3].cuda(), frames)
    assert base.stats["replay"] >= 3, base.stats
    lay = _runner(name, raw_layout=PADDED)
    assert lay.img is None and tuple(lay.raw.shape) == (1, 6, layout.image_bytes)
    b = _drive(lay, lambda f: padded[f % 3].cuda() if f % 2 else padded[f % 3].pin_memory(), frames)
    assert lay.stats == base.stats and lay.plan.key == P.plan_key((900, 1600), R50, "nv12", "jfif", layout) != base.plan.key
    _compare(a, b, name + " raw_layout")
    ptr = _runner(name, raw_layout=layout, raw_surfaces=True)
    assert ptr.img is None and ptr.raw.dtype == torch.int64 and tuple(ptr.raw.shape) == (1, 6)
    pools = Pools(padded)
    c = _drive(ptr, lambda f: [pools.frame(f)], frames)
    assert ptr.stats == base.stats, (ptr.stats, base.stats)
    _compare(a, c, name + " raw_surfaces")
    # refused before anything is enqueued: a tensor in place of the list, a host surface, a short surface, a missing one
    before = dict(ptr.stats)
    row = pools.frame(frames)
    metas = synth.frame_metas(1, frames)
    small = torch.zeros(layout.sample_end - 1, dtype=torch.uint8, device="cuda")
    for bad, err in ((padded[0].cuda(), ValueError), ([[t.cpu() for t in row]], RuntimeError), ([row[:5] + [small]], ValueError),
                     ([row[:5] + [None]], ValueError), ([row[:5]], ValueError)):
        with pytest.raises(err):
            ptr.step(bad, metas)
    with pytest.raises(ValueError, match="nv12 surface of 1600 x 900"):
        lay.step(tight[0].cuda(), metas)
    assert ptr.stats == before and len(getattr(ptr, "queue", [])) == 0 and lay.stats == base.stats


def test_runner_paused_stream_and_masked_camera_given_as_none():
    """Two independent streams as pointer lists without a layout (tight surfaces): stream 1 pauses for frames 3 and 4 (its row is
    None, or a row of None), stream 0 loses camera 2 in frames 2 .. 4 (None in its place). Equal to the tensor form."""
    tight, _, _ = _pictures()
    frames = 8
    active = [None, None, None, (True, False), (True, False), None, None, None]
    cameras = [None, None] + [[[True, True, False, True, True, True], [True] * 6]] * 3 + [None, None, None]
    base = _runner("PipelinedRunner", bs=2)
    both = lambda f: torch.cat([tight[f % 3], tight[(f + 1) % 3]]).cuda()   # noqa: E731
    a = _drive(base, both, frames, bs=2, active=active, cameras=cameras)
    ptr = _runner("PipelinedRunner", bs=2, raw_surfaces=True)
    held = []

    def feed(f):
        rows = [[tight[(f + s) % 3][0, c].cuda() for c in range(6)] for s in range(2)]
        held.append(rows)
        rows = [list(r) for r in rows]
        if cameras[f] is not None:
            rows[0][2] = None
        if active[f] is not None:
            rows[1] = None if f == 3 else [None] * 6
        return rows

    b = _drive(ptr, feed, frames, bs=2, active=active, cameras=cameras)
    assert ptr.stats == base.stats and ptr.stats["replay"] >= 2, (ptr.stats, base.stats)
    _compare(a, b, "paused + masked", streams=[(True, True) if m is None else m for m in active])
    assert [r is None for r in b[3][0]] == [False, True]


def test_runner_follows_a_changed_layout():
    """The decoder re-allocates its surfaces in the middle of a warm, replaying stream: tight for four frames, padded after.
    The plan key changes, every graph is dropped and captured again, and the results match the tight runner's throughout."""
    tight, padded, layout = _pictures()
    frames = 8
    base = _runner("FrameRunner")
    a = _drive(base, lambda f: tight[f % 3].cuda(), frames)
    r = _runner("FrameRunner")
    got = []
    for f in range(frames):
        if f == 4:
            assert r.graph is not None and r.stats["replay"] >= 2
            r.set_raw_layout(PADDED)
            assert r.graph is None and tuple(r.raw.shape) == (1, 6, layout.image_bytes)
            with pytest.raises(ValueError):
                r.step(tight[f % 3].cuda(), synth.frame_metas(1, f))        # the old form is no longer taken
        res = r.step((tight if f < 4 else padded)[f % 3].cuda(), synth.frame_metas(1, f))
        got.append((res, r.last_rec3d.clone(), r.last_rec2d.clone()))
    assert r.plan.key == P.plan_key((900, 1600), R50, "nv12", "jfif", layout) and r.stats["replay"] >= 4
    _compare(a, got, "layout change")


def test_changed_layout_is_refused_with_a_frame_in_flight():
    """A pipelined runner holds the last frame back: its staging buffers and graphs are not replaced under it. After `flush`
    the change is taken, and both staging buffers have the new shape."""
    tight, padded, layout = _pictures()
    r = _runner("PipelinedRunner")
    assert r.step(tight[0].cuda(), synth.frame_metas(1, 0)) is None and len(r.queue) == 1
    with pytest.raises(RuntimeError, match="flush"):
        r.set_raw_layout(PADDED)
    assert tuple(r.raw.shape) == (1, 6, 1350, 1600) and len(r.queue) == 1
    assert r.flush() is not None and not r.queue
    r.set_raw_layout(PADDED)
    assert [tuple(x.shape) for x in r.raws] == [(1, 6, layout.image_bytes)] * 2 and r.raw is r.raws[0]
    assert r.step(padded[1].cuda(), synth.frame_metas(1, 1)) is None
    assert r.flush() is not None and r.plan.key == P.plan_key((900, 1600), R50, "nv12", "jfif", layout)


def test_runner_options_need_raw_input():
    from simpb_amd import runner
    model = _model()
    for cls in (runner.FrameRunner, runner.PipelinedRunner, runner.SplitPipelinedRunner):
        for kw in (dict(raw_layout=PADDED), dict(raw_surfaces=True)):
            with pytest.raises(ValueError, match="raw_input"):
                cls(model, 1, (256, 704), device=torch.device("cuda"), **kw)
    with pytest.raises(ValueError, match="rows overlap"):
        runner.FrameRunner(model, 1, (256, 704), device=torch.device("cuda"), raw_input=(900, 1600), raw_format="nv12", raw_layout=dict(pitch=1599))
    with pytest.raises(ValueError, match="jfif"):
        runner.FrameRunner(model, 1, (256, 704), device=torch.device("cuda"), raw_input=(900, 1600), raw_format="p010")
    r = runner.FrameRunner(model, 1, (256, 704), device=torch.device("cuda"), raw_input=(900, 1600), raw_format="p010", raw_colour="bt709")
    assert tuple(r.raw.shape) == (1, 6, 1350, 3200)
