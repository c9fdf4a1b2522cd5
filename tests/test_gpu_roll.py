"""GPU: the per-camera mount roll inside the ingest's vertical pass (csrc/preprocess.hip: resample_cols_lut_roll_row) against
the numpy restatements (tests/preprocess_ref.py, then tests/roll_ref.py: both pinned to Pillow and to the reference's own
function by the host tests), and the runners' raw_roll / rolled raw_rig against the same runners fed the fp32 images those
restatements make. Integer arithmetic plus a table: every comparison is bit for bit. The kernel cases are a 36 x 50 source
to a 17 x 27 image (a width that is no multiple of 4: the last, partial group of pixels) and a 20 x 20 one (the transposes)."""
import ctypes

import numpy as np
import pytest
import torch

from simpb_amd import _lib
from simpb_amd import preprocess as P
from simpb_amd import synth
from tests import preprocess_ref as R
from tests import roll_ref as RR
from tests import surface_ref as S
from tests import yuv_ref as Y

pytestmark = pytest.mark.gpu

NORM = P.IMG_NORM_CFG
SRC = (36, 50)
AUG = dict(resize=0.6, crop=(1, 2, 28, 19))          # -> 17 x 27
SQUARE = dict(resize=0.6, crop=(1, 1, 21, 21))       # -> 20 x 20
ROLLS = (180, 90, 7.3, -31, 45, 359.5)


def pictures(n, seed=5):
    return np.random.RandomState(seed).randint(0, 256, (n,) + SRC + (3,)).astype(np.uint8)


def expected(bgr, aug, rolls, norm=NORM):
    """f16 [N, h, w, 4] of BGR pictures u8 [N, Hs, Ws, 3]: resize, crop, flip, the roll of image n (rolls[n % len]), normalise."""
    out = []
    for n, f in enumerate(bgr):
        u8 = RR.rotate(R.img_transform(f, aug), rolls[n % len(rolls)])
        out.append(R.normalise(u8, norm["mean"], norm["std"], norm.get("to_rgb", True)).astype(np.float16))
    x = np.stack(out)
    return torch.from_numpy(np.concatenate([x, np.zeros(x.shape[:3] + (1,), np.float16)], -1))


def assert_same_bits(got, want, what=""):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float16, (what, got.shape, want.shape)
    same = torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16))
    assert same, (what, int((got != want).sum()), "elements differ")


# ------------------------------------------------------------------------------------------------------------ uniform kernel
@pytest.mark.parametrize("to_rgb", [True, False])
@pytest.mark.parametrize("flip", [False, True])
def test_kernel_equals_restatement(flip, to_rgb):
    bgr = pictures(2)
    aug, norm = dict(AUG, flip=flip), dict(NORM, to_rgb=to_rgb)
    dev = torch.from_numpy(bgr).cuda()
    for roll in ROLLS:
        plan = P.ResamplePlan(SRC, aug, norm, roll=roll)
        assert plan.out_hw == (17, 27) and plan.rolled
        got = plan.run(dev)
        assert not got[..., 3].any()
        assert_same_bits(got, expected(bgr, aug, [roll], norm), (flip, to_rgb, roll))


@pytest.mark.parametrize("roll", [90, 270])
def test_square_crop_takes_the_transpose_integers(roll):
    bgr = pictures(1, 6)
    plan = P.ResamplePlan(SRC, SQUARE, roll=roll)
    assert plan.out_hw == (20, 20) and sorted(abs(int(v)) for v in plan.roll_ints[0, [0, 1, 3, 4]]) == [0, 0, 65536, 65536]
    got = plan.run(torch.from_numpy(bgr).cuda())
    assert_same_bits(got, expected(bgr, SQUARE, [roll]), roll)
    level = P.ResamplePlan(SRC, SQUARE).run(torch.from_numpy(bgr).cuda())
    assert_same_bits(got, torch.rot90(level, 1 if roll == 90 else 3, (1, 2)), roll)     # a pure permutation of the level pixels


def run_rows(plan, frames, rows):
    """The rolled entry point with a table of the test's own making (a plan only ever hands over its cameras' integers)."""
    plan.roll_ints, plan.rolls = np.ascontiguousarray(rows, np.int32), (0.0,) * len(rows)
    return plan.run(frames)


@pytest.mark.parametrize("flip", [False, True])
def test_identity_rows_give_the_level_bits(flip):
    bgr = pictures(3, 7)
    aug = dict(AUG, flip=flip)
    dev = torch.from_numpy(bgr).cuda()
    level = P.ResamplePlan(SRC, aug).run(dev)
    assert_same_bits(level, expected(bgr, aug, [0]))
    for cams in (1, 3, 16):
        got = run_rows(P.ResamplePlan(SRC, aug, roll=5), dev, [P.ROLL_IDENTITY] * cams)
        assert_same_bits(got, level, (flip, cams))


def test_three_images_three_rolls_in_one_launch():
    bgr = pictures(6, 8)
    rolls = [0, 180, -31]
    plan = P.ResamplePlan(SRC, AUG, roll=rolls)
    assert plan.roll_ints.shape == (3, 6)
    got = plan.run(torch.from_numpy(bgr).cuda().view(2, 3, *SRC, 3))     # [bs, cams]: image n takes roll n % 3
    assert_same_bits(got, expected(bgr, AUG, rolls))
    assert_same_bits(got[0::3], P.ResamplePlan(SRC, AUG).run(torch.from_numpy(bgr[0::3].copy()).cuda()), "the level camera")


def test_nv12():
    nv12 = Y.bgr_to_nv12(pictures(2, 9), "bt601")
    plan = P.ResamplePlan(SRC, dict(AUG, flip=True), frame_format="nv12", colour="bt601", roll=7.3)
    got = plan.run(torch.from_numpy(nv12).cuda())
    assert_same_bits(got, expected(Y.yuv420sp_to_bgr(nv12, "bt601"), dict(AUG, flip=True), [7.3]))


def test_padded_bgr_surfaces_through_an_address_table():
    bgr = pictures(3, 10)
    plan = P.ResamplePlan(SRC, AUG, layout=dict(pitch=50 * 3 + 7, image_bytes=36 * 157 + 11), roll=[-31, 0, 180])
    surfaces = [torch.from_numpy(S.pack(f, plan.surface, 0xEE)).cuda() for f in bgr]
    got = plan.run_surfaces(surfaces)
    assert_same_bits(got, expected(bgr, AUG, [-31, 0, 180]))


def test_p010():
    nv12 = Y.bgr_to_nv12(pictures(2, 11), "bt709")
    layout = P.SurfaceLayout(SRC, "p010")
    surf = S.pack(S.to_p010(nv12, np.random.RandomState(12)), layout)
    plan = P.ResamplePlan(SRC, AUG, frame_format="p010", colour="bt709", roll=45)
    got = plan.run(torch.from_numpy(surf).cuda().view(2, *plan.frame_shape))
    assert_same_bits(got, expected(S.p010_to_bgr(surf, layout, "bt709"), AUG, [45]))


# ---------------------------------------------------------------------------------------------------------------- rig kernel
RIG_ROLLS = (0, 180, -4.5)


def rolled_rig(rolls=RIG_ROLLS):
    """Three cameras of different source size and format to 24 x 40, with their BGR pictures and surfaces (two streams)."""
    specs = [((64, 96), dict(resize=0.5, crop=(4, 4, 44, 28)), "bgr", "jfif", None),
             ((100, 168), dict(resize=0.25, crop=(1, 1, 41, 25)), "nv12", "bt601", dict(pitch=176)),
             ((48, 80), dict(resize=0.5, crop=(0, 0, 40, 24), flip=True), "p010", "bt709", dict(pitch=192, luma_rows=56))]
    sources = [P.CameraSource(hw, aug, fmt, colour, layout, roll=r) for (hw, aug, fmt, colour, layout), r in zip(specs, rolls)]
    rng = np.random.RandomState(13)
    surfaces, bgrs = [], []
    for s in range(2):
        for src in sources:
            bgr = rng.randint(0, 256, src.src_hw + (3,)).astype(np.uint8)
            if src.frame_format == "nv12":
                nv12 = Y.bgr_to_nv12(bgr, src.colour)
                surf, bgr = S.pack(nv12, src.surface, 0xEE), Y.yuv420sp_to_bgr(nv12, src.colour)
            elif src.frame_format == "p010":
                surf = S.pack(S.to_p010(Y.bgr_to_nv12(bgr, src.colour), rng), src.surface, 0xEE)
                bgr = S.p010_to_bgr(surf, src.surface, src.colour)
            else:
                surf = S.pack(bgr, src.surface, 0xEE)
            surfaces.append(torch.from_numpy(surf).cuda())
            bgrs.append(bgr)
    return sources, surfaces, bgrs


def test_rig_kernel():
    sources, surfaces, bgrs = rolled_rig()
    rig = P.RigPlan(sources)
    assert rig.rolled and tuple(rig.roll_ints[0]) == P.ROLL_IDENTITY
    got = rig.run_surfaces(surfaces)
    want = torch.cat([expected(b[None], s.aug_config, [s.roll]) for b, s in zip(bgrs, sources * 2)])
    assert_same_bits(got, want)
    # the level camera's block equals the unrolled rig's (the level entry point)
    level_sources, _, _ = rolled_rig((0, 0, 0))
    level = P.RigPlan(level_sources)
    assert not level.rolled
    assert_same_bits(got[0::3], level.run_surfaces(surfaces)[0::3], "level camera")
    # a skipped image is all zeros, and no other block moves: each camera in turn
    for skip in (1, 3, 5):
        some = list(surfaces)
        some[skip] = None
        out = torch.full_like(got, 7.0)
        rig.run_surfaces(some, out)
        assert not out[skip].view(torch.int16).any(), skip
        keep = [i for i in range(6) if i != skip]
        assert_same_bits(out[keep], got[keep], skip)


# ------------------------------------------------------------------------------------------------- a refused call writes nothing
def test_refused_call_leaves_the_output_untouched():
    plan = P.ResamplePlan(SRC, AUG, roll=30).reserve(1, "cuda")
    d = plan._dev
    bgr = pictures(1, 14)
    src = torch.from_numpy(bgr).cuda()
    out = torch.full((1, 17, 27, 4), 7.0, dtype=torch.float16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    null = ctypes.c_void_p(0)
    ptrs = [p(out), p(src), null, p(d["mid"]), p(d["kx"]), p(d["xlo"]), p(d["xn"]), p(d["ky"]), p(d["ylo"]), p(d["yn"]), p(d["lut"])]
    good = [1, 36, 50, 17, 27, plan.taps_x, plan.taps_y, plan.src_row0, plan.src_rows, 0, 1, 0, 150, 0, 0, 0, 36 * 150, 0, 1, 0, 0, 0, 0]
    rows = plan.roll_ints.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = _lib.lib().simpb_preprocess_roll_nhwc4_f16
    assert fn(*ptrs, *good, None, 1, stream) == 1                                    # no table
    for cams in (0, 17, -1):
        assert fn(*ptrs, *good, rows, cams, stream) == 1
    for ints in (good[:3] + [8193] + good[4:], good[:4] + [8193] + good[5:], good[:6] + [65] + good[7:], [0] + good[1:],
                 good[:7] + [1, 36] + good[9:], good[:11] + [5] + good[12:], good[:12] + [149] + good[13:]):
        assert fn(*ptrs, *ints, rows, 1, stream) == 1
    assert fn(*([null] + ptrs[1:]), *good, rows, 1, stream) == 1
    assert fn(*(ptrs[:2] + [p(src)] + ptrs[3:]), *good, rows, 1, stream) == 1          # both forms of the images
    # the rig's rolled entry point: no table, and a camera the level form refuses
    sources, surfaces, _ = rolled_rig()
    rig = P.RigPlan(sources)
    rig_out = torch.full((3, 24, 40, 4), 7.0, dtype=torch.float16, device="cuda")
    rig.run_surfaces(surfaces[:3], torch.empty_like(rig_out))                         # (uploads the tables, makes `mid` and the address table)
    r = rig._dev
    args = lambda cams, n=3: (p(rig_out), p(r["table"]), p(r["mid"]), *(p(r[name]) for name in rig.TABLES), p(r["lut"]), cams, n, 3, 24, 40,   # noqa: E731
                              r["kx"].numel(), r["xlo"].numel(), r["ky"].numel(), r["ylo"].numel(), rig.mid_rows, 1)
    rig_rows = rig.roll_ints.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    rig_fn = _lib.lib().simpb_preprocess_rig_roll_nhwc4_f16
    assert rig_fn(*args(rig.descriptors()), None, stream) == 1
    assert rig_fn(*args(rig.descriptors(), 17), rig_rows, stream) == 1
    bad = rig.descriptors()
    bad[1].pitch = 167
    assert rig_fn(*args(bad), rig_rows, stream) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((rig_out == 7.0).all())
    assert fn(*ptrs, *good, rows, 1, stream) == 0     # (and the same buffers are taken when the arguments are right)
    assert rig_fn(*args(rig.descriptors()), rig_rows, stream) == 0
    torch.cuda.synchronize()
    assert_same_bits(out, expected(bgr, AUG, [30]))
    assert_same_bits(rig_out, rig.run_surfaces(surfaces[:3]))


# ------------------------------------------------------------------------------------------------------------------- runners
R50 = dict(resize=0.44, crop=(0, 140, 704, 396))
NUS = (900, 1600)
_cache = {}


def _model():
    from simpb_amd import configs, plugin
    cfg = configs.simpb_plus(anchor=synth.anchors(900))
    model = plugin.build_detector(cfg["model"]).eval()
    synth.load_procedural(model)
    model.cuda()
    model.fuse_conv_bn()
    model.half_backbone()
    return model


def _runner(name, **kw):
    from simpb_amd import runner
    return getattr(runner, name)(_model(), 1, (256, 704), capacity=1536, device=torch.device("cuda"), use_graph=True, **kw)


def _frame(f):
    """Frame f % 3 of the synthetic generator as (NV12 u8 [1, 6, 1350, 1600], the BGR pictures u8 [6, 900, 1600, 3] it holds)."""
    if ("nv12", f % 3) not in _cache:
        nv12 = Y.bgr_to_nv12(synth.raw_frames(1, f % 3)[0].numpy(), "jfif")
        _cache["nv12", f % 3] = (torch.from_numpy(nv12)[None], Y.yuv420sp_to_bgr(nv12, "jfif"))
    return _cache["nv12", f % 3]


def _witness(f, rolls):
    """f32 [1, 6, 3, 256, 704]: what the reference's host pipeline, its rotate included, makes of frame f's pictures."""
    key = ("fp32", f % 3, tuple(rolls))
    if key not in _cache:
        level = _cache.setdefault(("level", f % 3), [R.img_transform(b, R50) for b in _frame(f)[1]])
        x = [R.normalise(RR.rotate(u8, r), NORM["mean"], NORM["std"], True).transpose(2, 0, 1) for u8, r in zip(level, rolls)]
        _cache[key] = torch.from_numpy(np.ascontiguousarray(np.stack(x)))[None]
    return _cache[key]


def _drive(r, feed, frames, cameras=None):
    got = []
    keep = lambda res: got.append((res[0]["img_bbox"], r.last_rec3d.clone(), r.last_rec2d.clone()))   # noqa: E731
    for f in range(frames):
        res = r.step(feed(f), synth.frame_metas(1, f), **({} if cameras is None or cameras[f] is None else dict(cameras=cameras[f])))
        if res is not None:
            keep(res)
    if hasattr(r, "flush"):
        keep(r.flush())
    assert len(got) == frames
    return got


def _compare(a, b, name):
    for f, ((ra, a3, a2), (rb, b3, b2)) in enumerate(zip(a, b)):
        assert torch.equal(a3, b3), (name, f, "rec3d")
        assert torch.equal(a2, b2), (name, f, "rec2d")
        assert ra.keys() == rb.keys(), (name, f)
        for k in ra:
            x, y = ra[k], rb[k]
            if torch.is_tensor(x) or isinstance(x, np.ndarray):
                x, y = torch.as_tensor(x), torch.as_tensor(y)
                assert x.shape == y.shape and torch.equal(x, y), (name, f, k)
            else:
                assert np.array_equal(np.asarray(x), np.asarray(y)), (name, f, k)


def test_frame_runner_one_roll_per_camera_and_a_masked_rolled_camera():
    """raw_roll as a list, NV12 frames: cold frame, eager warm frame, replayed graphs; from frame 3 on camera 1 (rolled by 180
    degrees) is dropped through cameras=, and the run equals the witness under the same mask."""
    rolls = [0, 180, 3, -3, 0, 180]
    frames = 5
    lost = [[True, False, True, True, True, True]]
    cameras = [None] * 3 + [lost] * 2
    ref = _runner("FrameRunner")
    a = _drive(ref, lambda f: _witness(f, rolls).cuda(), frames, cameras)
    r = _runner("FrameRunner", raw_input=NUS, raw_format="nv12", raw_roll=rolls)
    b = _drive(r, lambda f: _frame(f)[0].cuda(), frames, cameras)
    assert r.stats == ref.stats and r.stats["replay"] >= 1, (r.stats, ref.stats)
    assert r.plan.rolled and r.plan.key == P.plan_key(NUS, R50, "nv12", "jfif", None, rolls) != P.plan_key(NUS, R50, "nv12", "jfif")
    _compare(a, b, "FrameRunner raw_roll list")
    # the roll reached the pictures: the level witness differs
    assert not torch.equal(_witness(0, rolls), _witness(0, [0] * 6))


def test_split_pipelined_runner_scalar_roll():
    rolls = [180] * 6
    frames = 7
    ref = _runner("SplitPipelinedRunner")
    a = _drive(ref, lambda f: _witness(f, rolls).pin_memory(), frames)
    r = _runner("SplitPipelinedRunner", raw_input=NUS, raw_format="nv12", raw_roll=180)
    b = _drive(r, lambda f: _frame(f)[0].pin_memory(), frames)
    assert r.stats == ref.stats and r.stats["replay"] >= 3, (r.stats, ref.stats)
    _compare(a, b, "SplitPipelinedRunner raw_roll=180")


def test_frame_runner_rig_with_a_rolled_camera_follows_set_raw_rig():
    """A rig of six NV12 cameras, camera 2 rolled by -4.5 degrees: cold, warm and replayed frames equal the witness; before the
    last frame the camera's roll becomes 3 degrees through set_raw_rig (the graphs are dropped), and that frame equals the
    witness of the new roll."""
    frames, switch = 5, 4
    rolls = {False: [0, 0, -4.5, 0, 0, 0], True: [0, 0, 3.0, 0, 0, 0]}
    rig = lambda now: [P.CameraSource(NUS, R50, "nv12", roll=x) for x in rolls[now]]   # noqa: E731
    ref = _runner("FrameRunner")
    a = _drive(ref, lambda f: _witness(f, rolls[f >= switch]).cuda(), frames)
    r = _runner("FrameRunner", raw_rig=rig(False))
    assert r.plan.rolled
    handed, got = [], []
    for f in range(frames):
        if f == switch:
            assert r.graph is not None and r.stats["replay"] >= 1
            old = r.plan
            r.set_raw_rig(rig(False))              # an equal key: nothing happens
            assert r.graph is not None and r.plan is old
            r.set_raw_rig(rig(True))
            assert r.graph is None and r.plan is not old and r.plan.rolled
        nv12 = _frame(f)[0][0]
        handed.append([nv12[c].cuda() for c in range(6)])     # (every surface stays referenced until the test ends)
        res = r.step([list(handed[-1])], synth.frame_metas(1, f))
        got.append((res[0]["img_bbox"], r.last_rec3d.clone(), r.last_rec2d.clone()))
    assert r.stats == ref.stats, (r.stats, ref.stats)
    _compare(a, got, "rolled rig + set_raw_rig")
