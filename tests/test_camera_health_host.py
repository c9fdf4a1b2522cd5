"""CPU: camera health without a device -- the configuration's validation, the refusals of the runners and of the three entry
points (validation runs before any HIP call), a runner built without the feature, and the numpy model (tests/health_ref.py)
alone on the frames the GPU runner tests use: every healthy image at least a factor 2 away from every threshold, every
doctored one at least a factor 2 inside its own. The figures are printed as `FIG` lines."""
import ctypes
import functools
import inspect
import types

import numpy as np
import pytest
import torch

from simpb_amd import health as H
from simpb_amd import synth
from simpb_amd.preprocess import IMG_NORM_CFG
from tests import health_ref as R
from tests import preprocess_ref as P

SRC = (300, 800)
AUG = dict(resize=0.44, crop=(0, 4, 352, 132))
HW = (128, 352)
EINVAL = 1


# ------------------------------------------------------------------------------------------------------------ configuration
def test_camera_health_defaults_and_validation():
    c = H.CameraHealth()
    assert (c.dark_below, c.bright_above, c.flat_below, c.frozen_after, c.act) == (16.0, 240.0, 2.0, 2, True)
    off = H.CameraHealth(dark_below=None, bright_above=None, flat_below=None, frozen_after=None, act=False)
    p = off.params()
    assert (p.check_dark, p.check_bright, p.check_flat, p.check_frozen, p.act) == (0, 0, 0, 0, 0)
    p = c.params(dict(mean=[1.0, 2.0, 3.0], std=[4.0, 5.0, 6.0]))
    assert list(p.mean) == [1.0, 2.0, 3.0] and list(p.std) == [4.0, 5.0, 6.0] and p.frozen_after == 2 and p.act == 1
    assert list(c.params().mean) == [float(v) for v in IMG_NORM_CFG["mean"]]
    for bad in (dict(frozen_after=0), dict(frozen_after=-1), dict(frozen_after=1.5), dict(frozen_after=True), dict(dark_below="low"),
                dict(dark_below=float("nan")), dict(bright_above=float("inf")), dict(flat_below=-1.0), dict(act=1),
                dict(dark_below=200.0, bright_above=100.0), dict(dark_below=True)):
        with pytest.raises(ValueError, match="camera_health"):
            H.CameraHealth(**bad)
    assert H.CameraHealth.make(c) is c and H.CameraHealth.make(dict(frozen_after=3)).frozen_after == 3
    with pytest.raises(ValueError):
        H.CameraHealth.make("on")
    assert H.describe(H.DARK | H.FROZEN) == ("dark", "frozen") and H.describe(0) == ()
    assert (H.DARK, H.BRIGHT, H.FLAT, H.FROZEN, H.FAIL_OPEN, H.NONFINITE) == (R.DARK, R.BRIGHT, R.FLAT, R.FROZEN, R.FAIL_OPEN, R.NONFINITE)


# ------------------------------------------------------------------------------------------------------------------ runners
@functools.lru_cache(maxsize=None)
def _cpu_model():
    from tests.helpers import build_product_head
    head = build_product_head(dict(image_wh=(176, 64), num_anchor=48, num_temp=32, num_output=20, bs=1), "cpu")
    return types.SimpleNamespace(head=head, parameters=head.parameters)


def _runner(**kw):
    from simpb_amd.runner import FrameRunner
    return FrameRunner(_cpu_model(), 1, (64, 176), capacity=128, device=torch.device("cpu"), use_graph=False, **kw)


def test_every_runner_takes_the_keyword_and_none_is_the_default():
    from simpb_amd import runner
    assert inspect.signature(runner.FrameRunner.__init__).parameters["camera_health"].default is None
    for cls in (runner.PipelinedRunner, runner.SplitPipelinedRunner):   # (they pass FrameRunner's arguments through)
        assert "camera_health" not in vars(cls) and issubclass(cls, runner.FrameRunner)


def test_runner_refusals():
    with pytest.raises(ValueError, match="raw frames"):   # tensor input
        _runner(camera_health=H.CameraHealth())
    with pytest.raises(ValueError, match="frozen_after"):
        _runner(raw_input=SRC, camera_health=dict(frozen_after=0))
    with pytest.raises(ValueError, match="camera_health"):
        _runner(raw_input=SRC, camera_health="yes")


def test_a_runner_without_camera_health_has_nothing_of_it():
    r = _runner(raw_input=SRC)
    assert r.health is None and r.health_slots is None and r.health_dev_state is None and r.last_health is None
    assert not r.cam_masked and "health_dropped" not in r.stats
    assert not hasattr(r, "health_params")
    assert r._health_launches(0) is None
    with pytest.raises(ValueError):
        r.health_state()
    on = _runner(raw_input=SRC, camera_health=dict(frozen_after=3))
    assert on.cam_masked and on.stats["health_dropped"] == 0 and on.health.frozen_after == 3
    hs = on.health_slots
    assert len(hs) == 1 and hs[0]["partials"].numel() * 8 == H.partials_bytes(6, 64, 176)
    assert tuple(hs[0]["cam_eff"].shape) == tuple(hs[0]["flags"].shape) == (1, 6) and bool(hs[0]["cam_eff"].all())
    assert tuple(on.health_dev_state.shape) == (1, 6, 2) and not bool(on.health_dev_state.any())


# ------------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_refuse_bad_arguments_without_a_device():
    from simpb_amd import _lib
    lib = _lib.lib()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    size = lib.simpb_image_health_partials_bytes
    assert size(6, 256, 704) == 6 * 64 * 26 * 8 and size(1, 8, 8) == 64 * 26 * 8 and size(65535, 16384, 16384) == 65535 * 64 * 26 * 8
    for bad in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 7, 8), (1, 8, 7), (1, 16385, 8), (1, 8, 16385)):
        assert size(*bad) == EINVAL, bad
        assert lib.simpb_image_health_stats(p, p, *bad, null) == EINVAL, bad
    assert lib.simpb_image_health_stats(null, p, 1, 8, 8, null) == EINVAL
    assert lib.simpb_image_health_stats(p, null, 1, 8, 8, null) == EINVAL
    assert lib.simpb_image_health_stats(p, ctypes.c_void_p(4100), 1, 8, 8, null) == EINVAL   # images: 8-byte aligned
    assert lib.simpb_image_health_stats(ctypes.c_void_p(4100), p, 1, 8, 8, null) == EINVAL
    with pytest.raises(ValueError):
        H.partials_bytes(1, 4, 4)

    ok = H.CameraHealth().params()
    verdict = lambda ptrs=(p, p, p, p), params=ok, sizes=(2, 6, 128, 352): lib.simpb_camera_health_verdict(   # noqa: E731
        *ptrs, null, null, params, *sizes, null)
    for k in range(4):   # cam_out, flags, state, partials
        assert verdict(ptrs=tuple(null if i == k else p for i in range(4))) == EINVAL, k
    for sizes in ((0, 6, 128, 352), (2, 0, 128, 352), (2, 65, 128, 352), (2, 6, 7, 352), (2, 6, 128, 4), (65536, 1, 8, 8), (2000, 40, 8, 8)):
        assert verdict(sizes=sizes) == EINVAL, sizes
    assert verdict(ptrs=(p, p, ctypes.c_void_p(4100), p)) == EINVAL
    bad = H.CameraHealth().params()
    bad.frozen_after = 0
    assert verdict(params=bad) == EINVAL
    bad = H.CameraHealth().params()
    bad.dark_below = float("nan")
    assert verdict(params=bad) == EINVAL
    bad = H.CameraHealth().params(dict(mean=[0, 0, 0], std=[1, 0, 1]))
    assert verdict(params=bad) == EINVAL
    assert lib.simpb_abi_version() == 7


# -------------------------------------------------------------------------------------------------------------- the model
def test_model_statistics_do_not_depend_on_how_the_image_is_cut():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((13, 21, 4)) * 50).astype(np.float16)
    x[3, 4, 1], x[12, 20, 2], x[0, 0, 3] = np.inf, np.nan, np.nan
    st, rows = R.stats(x), R.partial_rows(x)
    back = R.reduce_rows(rows)
    assert np.array_equal(st["S"], back["S"]) and st["hash"] == back["hash"] and st["nonfinite"] == back["nonfinite"] == 2
    again = R.reduce_rows(R.pack_rows(st))
    assert np.array_equal(st["S"], again["S"]) and st["hash"] == again["hash"] and again["nonfinite"] == 2
    y = x.copy()
    y[..., 3] = 0
    assert np.array_equal(R.partial_rows(y), rows)
    y = x.copy()
    y[0, 0, :3], y[0, 1, :3] = x[0, 1, :3], x[0, 0, :3]
    sw = R.stats(y)
    assert np.array_equal(sw["S"], st["S"]) and sw["hash"] != st["hash"]
    # splitmix64's finaliser on a known input (the first output of the generator seeded with 0)
    assert int(R.mix(np.uint64(0x9E3779B97F4A7C15))) == 0xE220A8397B1DCDAF


@functools.lru_cache(maxsize=None)
def frame_images(f):
    """f16 [6, 128, 352, 4]: what the ingest makes of synth.raw_frames(1, f, SRC) (tests/preprocess_ref.py)."""
    return P.nhwc4_f16(synth.raw_frames(1, f, SRC).numpy(), AUG, IMG_NORM_CFG)


def doctored(kind, like, seed=0):
    """u8 [300, 800, 3] source frames of the GPU runner tests' doctored cameras."""
    if kind == "dark":
        return np.zeros_like(like)
    if kind == "bright":
        return np.full_like(like, 255)
    if kind == "grey":
        return np.full_like(like, 128)
    assert kind == "flat"
    return (128 + np.random.default_rng(seed).integers(-1, 2, like.shape)).astype(np.uint8)


def _figures(img):
    level, cells = R.levels(R.stats(img), HW, IMG_NORM_CFG["mean"], IMG_NORM_CFG["std"])
    return float(level), float(cells.max() - cells.min())


def _headroom(level):
    """What bright_above is a factor away in: the distance to full scale. A level cannot exceed 255, so against a threshold
    near the top "a factor 2" says something only about what is left above (dark_below and flat_below start from 0)."""
    return 255.0 - level


def test_margins_of_the_frames_the_gpu_tests_use():
    c = H.CameraHealth()
    lo, hi, worst = 1e9, -1e9, 1e9
    for f in range(3):
        for cam, img in enumerate(frame_images(f)):
            level, spread = _figures(img)
            print(f"FIG healthy frame {f} camera {cam}: L = {level:.4f}, cell spread = {spread:.4f}")
            lo, hi, worst = min(lo, level), max(hi, level), min(worst, spread)
            assert level >= 2 * c.dark_below and _headroom(level) >= 2 * _headroom(c.bright_above), (f, cam, level)
            assert spread >= 2 * c.flat_below, (f, cam, spread)
    print(f"FIG healthy: L in [{lo:.4f}, {hi:.4f}], smallest cell spread {worst:.4f} against flat_below = {c.flat_below}")
    like = synth.raw_frames(1, 0, SRC).numpy()[0, 0]
    for kind in ("dark", "grey", "bright", "flat"):
        img = P.nhwc4_f16(doctored(kind, like)[None], AUG, IMG_NORM_CFG)[0]
        level, spread = _figures(img)
        print(f"FIG doctored {kind}: L = {level:.4f}, cell spread = {spread:.4f}")
        assert spread <= c.flat_below / 2, (kind, spread)
        if kind == "dark":
            assert level <= c.dark_below / 2
        elif kind == "bright":
            assert _headroom(level) <= _headroom(c.bright_above) / 2
        else:
            assert level >= 2 * c.dark_below and _headroom(level) >= 2 * _headroom(c.bright_above)
    # distinct frames hash apart, the same bytes hash the same
    hashes = {int(R.stats(img)["hash"]) for f in range(3) for img in frame_images(f)}
    assert len(hashes) == 18
    assert R.stats(frame_images(1)[2])["hash"] == R.stats(frame_images(1)[2].copy())["hash"]
