"""CPU: the host side of the per-camera mount roll (the reference's `img.rotate(rotate)`, augment.py:92,105). The numpy
restatement (tests/roll_ref.py) against the reference's own function (tests/golden/roll.npz, tools/golden/gen_roll_golden.py)
and against Pillow; the product's six integers (simpb_amd/preprocess.py:roll_integers) against that restatement; the
matrices, the keys, and every refusal that needs no device. Every image comparison is byte for byte."""
import ctypes
import functools
import types

import numpy as np
import pytest

from simpb_amd import _lib
from simpb_amd import preprocess as P
from tests import preprocess_ref as R
from tests import roll_ref as RR
from tests.helpers import load_golden

R50 = dict(resize=0.44, crop=(0, 140, 704, 396))
SIZES = ((256, 704), (17, 23), (9, 16), (32, 32))
ANGLES = (0, 360, 180, 90, -90, 1, -1, 0.5, 5.4, 45, 89.9, 90.1, 135, 179.9, 181, 359.5, -17.25, 1e-9)


def golden_cases():
    g = load_golden("roll.npz")
    for i in range(int(g["num_cases"])):
        aug = dict(resize=float(g[f"case{i}_resize"]), flip=bool(g[f"case{i}_flip"]))
        if g[f"case{i}_crop"].size:
            aug["crop"] = tuple(int(v) for v in g[f"case{i}_crop"])
        yield i, g[f"img{int(g[f'case{i}_source'])}"], aug, float(g[f"case{i}_rotate"]), g[f"case{i}_out"], g[f"case{i}_matrix"]


def test_fixture_holds_the_cases_asked_for():
    cases = list(golden_cases())
    assert len(cases) == 6 * 6 + 2
    assert sorted({c[3] for c in cases[:36]}) == sorted((180, 90, 7.5, -3.25, 45, 0.2))
    assert [c[3] for c in cases[36:]] == [90, 270] and all(c[4].shape[0] == c[4].shape[1] for c in cases[36:])
    assert any(c[2]["flip"] for c in cases) and any(not c[2]["flip"] for c in cases)
    # the roll does something: no fixture image is the level one (0.2 degrees moves no pixel of images this small by half a pixel)
    assert all(not np.array_equal(R.img_transform(img, aug), want) for _, img, aug, roll, want, _ in cases if roll != 0.2)


def test_restatement_equals_reference_golden():
    for i, img, aug, roll, want, _ in golden_cases():
        got = RR.rotate(R.img_transform(img, aug), roll)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (i, roll, int((got != want).sum()))


def test_product_integers_reproduce_reference_golden():
    for i, img, aug, roll, want, _ in golden_cases():
        plan = P.ResamplePlan(img.shape[:2], aug, roll=roll)
        assert plan.rolled and plan.roll_ints.shape == (1, 6) and plan.roll_ints.dtype == np.int32
        got = RR.gather(R.img_transform(img, aug), plan.roll_ints[0])
        assert np.array_equal(got, want), (i, roll, int((got != want).sum()))


@pytest.mark.parametrize("hw", SIZES)
def test_restatement_and_product_equal_pillow(hw):
    Image = pytest.importorskip("PIL.Image")
    img = np.random.RandomState(hw[0]).randint(0, 256, hw + (3,)).astype(np.uint8)
    for angle in ANGLES:
        want = np.asarray(Image.fromarray(img).rotate(angle))
        got = RR.rotate(img, angle)
        assert np.array_equal(got, want), (hw, angle, int((got != want).sum()))
        got = RR.gather(img, P.roll_integers(angle, hw))
        assert np.array_equal(got, want), (hw, angle, int((got != want).sum()))


def test_integers_of_the_named_cases():
    h, w = 256, 704
    assert P.roll_integers(0, (h, w)) == P.roll_integers(360, (h, w)) == P.roll_integers(-720.0, (h, w)) == P.ROLL_IDENTITY
    assert P.ROLL_IDENTITY == (65536, 0, 32768, 0, 65536, 32768)
    assert P.roll_integers(180, (h, w)) == (-65536, 0, (w << 16) - 32768, 0, -65536, (h << 16) - 32768)
    img = np.arange(5 * 5 * 3, dtype=np.uint8).reshape(5, 5, 3)
    assert np.array_equal(RR.gather(img, P.ROLL_IDENTITY), img)
    assert np.array_equal(RR.gather(img, P.roll_integers(90, (5, 5))), np.rot90(img, 1))      # the transposes: pure permutations
    assert np.array_equal(RR.gather(img, P.roll_integers(270, (5, 5))), np.rot90(img, 3))
    assert np.array_equal(RR.gather(img, P.roll_integers(-180, (5, 5))), img[::-1, ::-1])
    for six in (P.roll_integers(a, (8192, 8192)) for a in (45, 135.5, -0.1, 90, 180)):     # the largest image: int32, all six
        assert all(-2 ** 31 <= v < 2 ** 31 for v in six)


def test_matrices_equal_the_reference():
    for i, img, aug, roll, _, want in golden_cases():
        assert want.shape == (4, 4) and np.array_equal(want[3], [0, 0, 0, 1]) and np.array_equal(want[:3, 3], [0, 0, 0])
        got = P.ResamplePlan(img.shape[:2], aug, roll=roll).image_transform()
        assert got.dtype == np.float64 and got.shape == (3, 3) and np.abs(got - want[:3, :3]).max() <= 1e-12, (i, roll)
        got = P.RigPlan([P.CameraSource(img.shape[:2], aug, roll=roll)]).image_transforms()[0]
        assert np.abs(got - want[:3, :3]).max() <= 1e-12, (i, roll)
    # roll = 0: exactly what the rig returned before there was a roll (closed forms of tests/test_rig_ingest_host.py)
    for kw in (dict(), dict(roll=0), dict(roll=0.0)):
        s = P.CameraSource((64, 96), dict(resize=0.5, crop=(4, 4, 44, 28), flip=True), **kw)
        want = np.array([[-0.5, 0, 40 + 4], [0, 0.5, -4], [0, 0, 1]])
        assert np.array_equal(P.RigPlan([s]).image_transforms()[0], want)
        assert np.array_equal(P.ResamplePlan((64, 96), dict(resize=0.5, crop=(4, 4, 44, 28), flip=True), **kw).image_transform(), want)
    # one roll per camera: each camera's own matrix
    plan = P.ResamplePlan((64, 96), dict(resize=0.5), roll=[0, 30.0])
    assert np.array_equal(plan.image_transform(0), np.diag([0.5, 0.5, 1.0])) and not np.array_equal(plan.image_transform(1), plan.image_transform(0))


def test_keys():
    src = (900, 1600)
    # every key that existed keeps its value
    assert P.plan_key(src, R50) == (900, 1600, (704, 396), (0, 140, 704, 396), False, "bgr", None)
    assert P.plan_key(src, R50, "nv12", "bt601") == (900, 1600, (704, 396), (0, 140, 704, 396), False, "nv12", "bt601")
    padded = P.plan_key(src, R50, "nv12", "bt601", dict(pitch=1664))
    assert padded[:-1] == P.plan_key(src, R50, "nv12", "bt601") and padded[-1] == P.SurfaceLayout(src, "nv12", pitch=1664).key
    for args in ((src, R50), (src, R50, "nv12", "bt601"), (src, R50, "nv12", "bt601", dict(pitch=1664))):
        for level in (0, 0.0, 360, -360.0, 720, [0, 360, 0]):
            assert P.plan_key(*args, roll=level) == P.plan_key(*args), (args, level)
        assert P.ResamplePlan(args[0], args[1], None, *args[2:]).key == P.plan_key(*args)
        rolled = P.plan_key(*args, roll=5)
        assert rolled != P.plan_key(*args) and rolled[:-1] == P.plan_key(*args)
        assert rolled != P.plan_key(*args, roll=-5) and rolled == P.plan_key(*args, roll=365) and rolled == P.plan_key(*args, roll=5.0)
        assert P.plan_key(*args, roll=[0, 5]) != P.plan_key(*args, roll=[5, 0]) != rolled
    cam = P.CameraSource(src, R50)
    assert cam.key == P.plan_key(src, R50) + (0.44,) and P.CameraSource(src, R50, roll=360).key == cam.key
    assert P.CameraSource(src, R50, roll=5).key != cam.key and P.CameraSource(src, R50, roll=5).key != P.CameraSource(src, R50, roll=-5).key
    rig = P.RigPlan([cam, P.CameraSource(src, R50, roll=180)])
    assert rig.key != P.RigPlan([cam, cam]).key and rig.key != P.RigPlan([P.CameraSource(src, R50, roll=180), cam]).key
    # a level plan or rig carries no integers (it calls the level entry points); a mixed rig has identity rows
    assert not P.ResamplePlan(src, R50).rolled and P.ResamplePlan(src, R50, roll=720).roll_ints is None
    assert not P.RigPlan([cam, cam]).rolled and P.RigPlan([cam, cam]).roll_ints is None
    assert rig.rolled and rig.roll_ints.shape == (2, 6) and tuple(rig.roll_ints[0]) == P.ROLL_IDENTITY
    assert tuple(rig.roll_ints[1]) == P.roll_integers(180, (256, 704))
    mixed = P.ResamplePlan(src, R50, roll=[0, 180, 3])
    assert mixed.rolled and mixed.roll_ints.shape == (3, 6) and tuple(mixed.roll_ints[0]) == P.ROLL_IDENTITY
    # the 2D back-mapping table does not see the roll (the reference's decode_box2d does not)
    assert np.array_equal(rig.box2d_table()[0], rig.box2d_table()[1])


def test_plan_refusals():
    src = (900, 1600)
    for aug in (dict(resize=0.44, rotate=5), dict(resize=0.44, rotate=180)):   # the aug_config's own rotate: refused as ever
        with pytest.raises(NotImplementedError):
            P.ResamplePlan(src, aug)
        with pytest.raises(NotImplementedError):
            P.ResamplePlan(src, aug, roll=5)
        with pytest.raises(NotImplementedError):
            P.CameraSource(src, aug, roll=5)
    for bad in (float("nan"), float("inf"), -float("inf"), True, False, np.bool_(True), "5", None, 1j, [1.0, float("nan")], [], [0.0] * 17,
                [[1.0]]):
        with pytest.raises(ValueError):
            P.ResamplePlan(src, R50, roll=bad)
        with pytest.raises(ValueError):
            P.plan_key(src, R50, roll=bad)
        with pytest.raises(ValueError):
            P.CameraSource(src, R50, roll=bad)
    assert P.ResamplePlan(src, R50, roll=np.float32(2.5)).rolls == (2.5,) and P.CameraSource(src, R50, roll=3).roll == 3.0
    # above 8192 a side Pillow may leave its fixed-point path: refused where a camera is rolled, taken where none is
    tall = dict(resize=1, crop=(0, 0, 4, 8193))
    assert P.ResamplePlan((8193, 4), tall).out_hw == (8193, 4) and P.ResamplePlan((8193, 4), tall, roll=360).out_hw == (8193, 4)
    with pytest.raises(ValueError, match="8192"):
        P.ResamplePlan((8193, 4), tall, roll=1)
    with pytest.raises(ValueError, match="8192"):
        P.RigPlan([P.CameraSource((8193, 4), tall, roll=180)])
    with pytest.raises(ValueError, match="8192"):
        P.roll_integers(90, (16, 8193))
    assert P.roll_integers(90, (8192, 8192))[0] == 0


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


def test_runner_takes_and_refuses_raw_roll():
    import inspect
    from simpb_amd import runner
    assert inspect.signature(runner.FrameRunner.__init__).parameters["raw_roll"].default is None
    for cls in (runner.PipelinedRunner, runner.SplitPipelinedRunner):   # (they pass FrameRunner's arguments through)
        assert issubclass(cls, runner.FrameRunner)
    src = (160, 400)
    cams = _cpu_model().head.num_cams
    assert _runner(raw_input=src).raw_roll == 0.0
    assert _runner(raw_input=src, raw_roll=180).raw_roll == 180.0
    assert _runner(raw_input=src, raw_format="nv12", raw_roll=[1.5] * cams).raw_roll == (1.5,) * cams
    with pytest.raises(ValueError, match="raw_input"):
        _runner(raw_roll=5.0)                                                   # tensor input
    with pytest.raises(ValueError, match="raw_input"):
        _runner(raw_roll=[0.0] * cams)
    rig = [P.CameraSource(src, dict(resize=0.44, crop=(0, 6, 176, 70)), roll=2.0)] * cams
    with pytest.raises(ValueError, match="CameraSource brings its own"):
        _runner(raw_rig=rig, raw_roll=5.0)
    for n in (cams - 1, cams + 1, 0):
        with pytest.raises(ValueError, match="raw_roll lists"):
            _runner(raw_input=src, raw_roll=[1.0] * n)
    for bad in (float("nan"), float("inf"), True, "3", [1.0] * (cams - 1) + [float("nan")], [1.0] * (cams - 1) + [True]):
        with pytest.raises(ValueError):
            _runner(raw_input=src, raw_roll=bad)


# ------------------------------------------------------------------------------------------------------------- entry points
NULL, OK = ctypes.c_void_p(0), ctypes.c_void_p(64)
SIX = ctypes.c_int * 6


def _rows(n=1):
    return (ctypes.c_int * (6 * n))(*(P.ROLL_IDENTITY * n))


def test_uniform_entry_point_refuses_before_any_hip_call():
    """Validation precedes any HIP call, so it is checkable without a device. The base arguments are those of
    tests/test_plane_ingest_host.py (a consistent padded yuv420p batch) with a good table, so each refusal has the one cause its
    line names: first the roll's own, then each one the level form makes."""
    fn = _lib.lib().simpb_preprocess_roll_nhwc4_f16
    cb, cr = 80 * 128 + 4, 80 * 128 + 4 + 32 * 56
    last = cr + 31 * 56 + 48
    ints = dict(num_images=2, src_height=64, src_width=96, out_height=32, out_width=48, taps_x=9, taps_y=9, src_row0=0, src_rows=64,
                flip=0, swap_rb=1, format=8, pitch=128, chroma_pitch=56, chroma_offset=cb, chroma2_offset=cr, image_stride=last,
                yoff=16, iy=76309, irv=104597, igu=-25675, igv=-53279, ibu=132201)
    names = ["out", "src", "image_table", "mid", "kx", "xlo", "xn", "ky", "ylo", "yn", "lut"]

    def call(ptrs=None, roll=_rows(2), roll_cams=2, **changed):
        vals = dict(ints, **changed)
        p = dict(dict.fromkeys(names, OK), image_table=NULL)
        p.update(ptrs or {})
        return fn(*[p[k] for k in names], *vals.values(), roll, roll_cams, NULL)

    # the roll's own refusals
    assert call(roll=None) == 1
    for n in (0, -1, 17, 1 << 20):
        assert call(roll=_rows(16), roll_cams=n) == 1, n
    assert call(out_height=8193) == 1 and call(out_height=65535) == 1 and call(out_width=8193) == 1
    # every refusal of the level form (tests/test_plane_ingest_host.py, line for line)
    for k in names:
        if k != "image_table":
            assert call({k: NULL}) == 1, k
    assert call(dict(src=OK, image_table=OK)) == 1 and call(dict(src=NULL, image_table=NULL)) == 1
    assert call(dict(src=NULL, image_table=ctypes.c_void_p(68))) == 1
    for code in (4, 5, 6, 7, 14, -1):
        assert call(format=code) == 1, code
    assert call(src_height=65, src_rows=65) == 1 and call(src_width=97) == 1 and call(iy=0) == 1
    assert call(pitch=95) == 1 and call(chroma_pitch=47) == 1
    assert call(chroma_offset=63 * 128 + 95) == 1 and call(chroma2_offset=63 * 128 + 95) == 1 and call(chroma2_offset=-1) == 1
    assert call(chroma2_offset=cb) == 1 and call(chroma2_offset=cb + 31 * 56 + 47) == 1
    assert call(chroma_offset=cr + 31 * 56 + 47, image_stride=30000) == 1
    assert call(image_stride=last - 1) == 1
    assert call(chroma_offset=cr + 32 * 56, image_stride=cr + 32 * 56 + 31 * 56 + 47) == 1
    one_plane = dict(chroma_pitch=0, chroma_offset=0, chroma2_offset=0)
    for code, px in ((9, 2), (10, 2), (11, 3), (12, 4), (13, 4)):
        base = dict(one_plane, format=code, pitch=96 * px + 5, image_stride=63 * (96 * px + 5) + 96 * px)
        assert call(**dict(base, pitch=96 * px - 1)) == 1, code
        assert call(**dict(base, image_stride=base["image_stride"] - 1)) == 1, code
        assert call(**dict(base, src_width=4098)) == 1 and call(**dict(base, num_images=0)) == 1
    for code in (9, 10):
        assert call(**dict(one_plane, format=code, src_width=95, pitch=400, image_stride=64 * 400)) == 1
        assert call(**dict(one_plane, format=code, pitch=400, image_stride=64 * 400, iy=0)) == 1
    assert call(format=1, chroma_pitch=95, chroma2_offset=0) == 1 and call(format=0, pitch=287) == 1
    assert call(format=3, pitch=257, chroma_pitch=256, chroma_offset=80 * 256, chroma2_offset=0, image_stride=30000) == 1
    assert call(out_width=2049) == 1 and call(taps_x=65) == 1 and call(taps_y=65) == 1 and call(src_row0=1) == 1
    assert call(dict(out=ctypes.c_void_p(72))) == 1 and call(dict(mid=ctypes.c_void_p(72))) == 1
    for k in ("num_images", "src_height", "src_width", "out_height", "out_width", "taps_x", "taps_y", "src_rows"):
        for bad in (0, -1):
            assert call(**{k: bad}) == 1, (k, bad)
    assert call(num_images=65536) == 1 and call(src_row0=-1) == 1


def _rig_sources():
    return [P.CameraSource((64, 96), dict(resize=0.5, crop=(4, 4, 44, 28))),
            P.CameraSource((100, 168), dict(resize=0.25, crop=(1, 1, 41, 25)), "nv12", layout=dict(pitch=176), roll=180),
            P.CameraSource((48, 80), dict(resize=0.5, crop=(0, 0, 40, 24), flip=True), "p010", "bt709", dict(pitch=192, luma_rows=56), roll=-4.5)]


def test_rig_entry_point_refuses_before_any_hip_call():
    rig = P.RigPlan(_rig_sources())
    fn = _lib.lib().simpb_preprocess_rig_roll_nhwc4_f16
    lens = (sum(k.size for k in rig.kx), 3 * 40, sum(k.size for k in rig.ky), 3 * 24, rig.mid_rows)
    rows = rig.roll_ints.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    def call(ptrs=(OK,) * 10, cams=None, n_cams=3, n_images=6, h=24, w=40, lens=lens, roll=rows, changed=None):
        cams = rig.descriptors() if cams is None else cams
        for (c, field), v in (changed or {}).items():
            setattr(cams[c], field, v)
        return fn(*ptrs, cams, n_cams, n_images, h, w, *lens, 1, roll, None)

    # the roll's own refusals
    assert call(roll=None) == 1
    assert call(h=8193) == 1 and call(w=8193) == 1
    # what the level rig entry point refuses (tests/test_rig_ingest_host.py, tests/test_plane_ingest_host.py)
    for n_cams, n_images in ((0, 6), (17, 17), (3, 5), (3, 0), (-1, 6)):
        assert call(n_cams=n_cams, n_images=n_images) == 1, (n_cams, n_images)
    assert fn(*(OK,) * 10, None, 3, 6, 24, 40, *lens, 1, rows, None) == 1
    for i in range(10):                                                      # every pointer (the table is one of them)
        assert call(ptrs=(OK,) * i + (NULL,) + (OK,) * (9 - i)) == 1, i
    assert call(ptrs=(ctypes.c_void_p(72),) + (OK,) * 9) == 1 and call(ptrs=(OK, ctypes.c_void_p(68)) + (OK,) * 8) == 1
    for i in range(5):                                                       # the table lengths
        assert call(lens=lens[:i] + (0,) + lens[i + 1:]) == 1, i
        assert call(lens=lens[:i] + (lens[i] - 1,) + lens[i + 1:]) == 1, i
    assert call(w=2049) == 1 and call(h=0) == 1 and call(w=0) == 1
    bad = [{(1, "pitch"): 167}, {(1, "chroma_pitch"): 167}, {(1, "src_width"): 169}, {(1, "src_height"): 101}, {(1, "iy"): 0},
           {(2, "pitch"): 159}, {(2, "chroma_offset"): 1}, {(0, "format"): 6}, {(0, "format"): 14}, {(0, "format"): -1},
           {(0, "taps_x"): 65}, {(0, "taps_y"): 0}, {(0, "src_row0"): -1}, {(0, "src_rows"): 65}, {(0, "src_width"): 4097},
           {(1, "kx_offset"): -1}, {(1, "kx_offset"): 0}, {(1, "x_offset"): 0}, {(1, "ky_offset"): 0}, {(1, "y_offset"): 0},
           {(1, "mid_row"): 0}, {(2, "mid_row"): rig.mid_rows}, {(2, "ky_offset"): lens[2]}]
    for changed in bad:
        assert call(changed=changed) == 1, changed
