"""CPU: the camera frame ingest's host side. The numpy restatement of the resampler (tests/preprocess_ref.py) against the
reference's own function (tests/golden/preprocess.npz, tools/golden/gen_preprocess_golden.py) and against Pillow; the
product's tables (simpb_amd/preprocess.py) against that restatement; the C entry's argument checks. Every comparison is
byte for byte."""
import ctypes
import os
import re

import numpy as np
import pytest

from simpb_amd import preprocess as P
from tests import preprocess_ref as R
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R50 = dict(resize=0.44, crop=(0, 140, 704, 396))
R101 = dict(resize=0.88, crop=(0, 280, 1408, 792))


def golden_cases():
    g = load_golden("preprocess.npz")
    for i in range(int(g["num_cases"])):
        aug = dict(resize=float(g[f"case{i}_resize"]), flip=bool(g[f"case{i}_flip"]))
        if g[f"case{i}_crop"].size:
            aug["crop"] = tuple(int(v) for v in g[f"case{i}_crop"])
        yield i, g[f"case{i}_img"], aug, g[f"case{i}_out"]


def apply_plan(plan, img):
    """The device kernels' arithmetic driven by the PRODUCT's tables, in numpy: what csrc/preprocess.hip computes before
    the normalisation table (u8 [h, w, 3])."""
    src = img.astype(np.int64)
    h, w = plan.out_hw
    rows = src[plan.src_row0:plan.src_row0 + plan.src_rows]
    mid = np.empty((plan.src_rows, w, 3), np.uint8)
    for j in range(w):
        jj = w - 1 - j if plan.flip else j
        acc = np.full((plan.src_rows, 3), 1 << 21, np.int64)
        for t in range(plan.xn[jj]):
            acc += rows[:, plan.xlo[jj] + t] * int(plan.kx[jj, t])
        mid[:, j] = np.clip(acc >> 22, 0, 255)
    out = np.empty((h, w, 3), np.uint8)
    m = mid.astype(np.int64)
    for y in range(h):
        acc = np.full((w, 3), 1 << 21, np.int64)
        for t in range(plan.yn[y]):
            acc += m[plan.ylo[y] - plan.src_row0 + t] * int(plan.ky[y, t])
        out[y] = np.clip(acc >> 22, 0, 255)
    return out


def test_restatement_equals_reference_golden():
    n = 0
    for i, img, aug, want in golden_cases():
        got = R.img_transform(img, aug)
        assert got.shape == want.shape and np.array_equal(got, want), (i, int((got != want).sum()))
        n += 1
    assert n >= 5


def test_plan_tables_reproduce_reference_golden():
    for i, img, aug, want in golden_cases():
        plan = P.ResamplePlan(img.shape[:2], aug)
        got = apply_plan(plan, img)
        assert got.shape == want.shape and np.array_equal(got, want), (i, int((got != want).sum()))


@pytest.mark.parametrize("dims", [(704, 396), (1408, 792)])
@pytest.mark.parametrize("kind", ["random", "gradient"])
def test_restatement_equals_pillow(dims, kind):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(7)
    if kind == "random":
        img = rng.randint(0, 256, (900, 1600, 3)).astype(np.uint8)
    else:
        y, x = np.mgrid[0:900, 0:1600]
        img = np.stack([(x * 255 // 1599), (y * 255 // 899), ((x + y) * 255 // 2498)], -1).astype(np.uint8)
    want = np.asarray(Image.fromarray(img).resize(dims))
    assert np.array_equal(want, np.asarray(Image.fromarray(img).resize(dims, Image.BICUBIC)))
    got = R.resize(img, dims)
    assert got.shape == want.shape and int((got != want).sum()) == 0


def test_plan_shipped_configurations():
    for aug, rows, taps, hw in ((R50, (315, 899), 11, (256, 704)), (R101, (316, 899), 7, (512, 1408))):
        plan = P.ResamplePlan((900, 1600), aug)
        assert plan.out_hw == hw and plan.resize_dims == (hw[1], aug["crop"][3])
        assert (plan.src_row0, plan.src_row0 + plan.src_rows - 1) == rows
        assert plan.taps_x == taps and plan.taps_y == taps
        assert plan.kx.shape == (hw[1], taps) and plan.ky.shape == (hw[0], taps)
        for k in (plan.kx, plan.ky):   # the int32 accumulator bound, every uploaded row
            assert ((1 << 21) + 255 * np.abs(k.astype(np.int64)).sum(1) < (1 << 31)).all()
        # the tables are the restatement's, entry for entry
        for lo, n, k, tab in ((plan.xlo, plan.xn, plan.kx, R.axis_table(1600, plan.resize_dims[0])[aug["crop"][0]:aug["crop"][2]]),
                              (plan.ylo, plan.yn, plan.ky, R.axis_table(900, plan.resize_dims[1])[aug["crop"][1]:aug["crop"][3]])):
            assert len(tab) == len(lo)
            for i, (first, coeff) in enumerate(tab):
                assert lo[i] == first and n[i] == len(coeff) and k[i, :n[i]].tolist() == coeff and not k[i, n[i]:].any()
        assert (plan.xlo >= 0).all() and (plan.xlo + plan.xn <= 1600).all() and (plan.ylo + plan.yn <= 900).all()


def test_plan_identity_and_defaults():
    plan = P.ResamplePlan((256, 704), dict(resize=1))
    assert plan.resize_dims == (704, 256) and plan.crop == (0, 0, 704, 256) and plan.out_hw == (256, 704) and not plan.flip
    assert plan.taps_x == 1 and plan.taps_y == 1 and (plan.kx == 1 << 22).all() and (plan.ky == 1 << 22).all()
    assert np.array_equal(plan.xlo, np.arange(704)) and np.array_equal(plan.ylo, np.arange(256))
    assert (plan.src_row0, plan.src_rows) == (0, 256)
    img = np.random.RandomState(1).randint(0, 256, (256, 704, 3)).astype(np.uint8)
    assert np.array_equal(apply_plan(plan, img), img)
    # augment.py:88-90: resize_dims = (int(W * resize), int(H * resize)), crop = the whole resized image
    plan = P.ResamplePlan((900, 1600), dict(resize=0.44))
    assert plan.resize_dims == (int(1600 * 0.44), int(900 * 0.44)) == (704, 396) and plan.crop == (0, 0, 704, 396)
    plan = P.ResamplePlan((177, 321), dict(resize=0.47, flip=True))
    assert plan.resize_dims == (int(321 * 0.47), int(177 * 0.47)) and plan.flip
    assert P.ResamplePlan((900, 1600), dict(resize=0.3, resize_dims=(704, 396))).resize_dims == (704, 396)
    assert P.plan_key((900, 1600), R50) == P.plan_key((900, 1600), dict(resize=0.44, crop=[0, 140, 704, 396], flip=False, rotate=0))
    assert P.plan_key((900, 1600), R50) != P.plan_key((900, 1600), dict(resize=0.44, crop=(0, 139, 704, 395)))


def test_plan_error_cases_raise_before_any_launch():
    torch = pytest.importorskip("torch")
    with pytest.raises(NotImplementedError):
        P.ResamplePlan((900, 1600), dict(resize=0.44, rotate=5))
    for crop in ((0, 140, 705, 396), (0, 140, 704, 397), (-1, 0, 704, 396), (10, 10, 10, 20)):
        with pytest.raises(ValueError):
            P.ResamplePlan((900, 1600), dict(resize=0.44, crop=crop))
    plan = P.ResamplePlan((90, 160), dict(resize=0.5))
    # input checks come first: they raise on CPU tensors, where a launch could only fail differently
    with pytest.raises(ValueError):
        plan.run(torch.zeros(2, 90, 160, 3))                          # not uint8
    with pytest.raises(ValueError):
        plan.run(torch.zeros(2, 90, 160, 4, dtype=torch.uint8))        # not [..., 3]
    with pytest.raises(ValueError):
        plan.run(torch.zeros(2, 3, 90, 160, dtype=torch.uint8))        # planar, not interleaved
    with pytest.raises(RuntimeError, match="GPU only"):
        plan.run(torch.zeros(2, 90, 160, 3, dtype=torch.uint8))        # right form, no device: an error, no fallback


@pytest.mark.parametrize("to_rgb", [True, False])
def test_normalise_table(to_rgb):
    cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=to_rgb)
    mean = np.asarray(cfg["mean"], np.float32)
    stdinv = (1.0 / np.asarray(cfg["std"], np.float64)).astype(np.float32)
    want = ((np.arange(256, dtype=np.float32)[None] - mean[:, None]) * stdinv[:, None]).astype(np.float16)
    plan = P.ResamplePlan((64, 64), dict(resize=1), cfg)
    assert plan.lut.dtype == np.float16 and plan.lut.shape == (3, 256)
    assert np.array_equal(plan.lut.view(np.uint16), want.view(np.uint16))
    assert plan.swap_rb == to_rgb
    # table + channel order == the fp32 pipeline cast to f16, for every byte value in every channel
    img = np.stack([np.arange(256, dtype=np.uint8)] * 3, -1).reshape(16, 16, 3).copy()
    img[..., 1] = img[::-1, :, 1]
    img[..., 2] = img[:, ::-1, 2]
    ref = R.normalise(img, cfg["mean"], cfg["std"], to_rgb).astype(np.float16)
    got = np.stack([plan.lut[c][img[..., 2 - c if to_rgb else c]] for c in range(3)], -1)
    assert np.array_equal(got.view(np.uint16), ref.view(np.uint16))
    assert np.array_equal(P.normalise_lut(None), P.ResamplePlan((8, 8), None).lut)   # default: the shipped config's


def test_c_entry_declared_and_rejects_bad_arguments():
    """The new symbol is in the header, and its argument checks run before any HIP call (no device here)."""
    text = open(os.path.join(ROOT, "include", "simpb_hip.h")).read()
    assert re.search(r"\bint\s+simpb_preprocess_u8_nhwc4_f16\s*\(", text) and re.search(r"\bint\s+simpb_preprocess_mid_pitch\s*\(", text)
    cap = int(re.search(r"#define\s+SIMPB_PREPROCESS_MAX_TAPS\s+(\d+)", text).group(1))
    from simpb_amd import _lib
    h = _lib.lib()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(256)
    ptrs = [p] * 10
    good = [6, 900, 1600, 256, 704, 11, 11, 315, 585, 0, 1]
    call = lambda ptrs, ints: h.simpb_preprocess_u8_nhwc4_f16(*ptrs, *ints, null)   # noqa: E731
    for i in range(10):                                     # every pointer
        assert call(ptrs[:i] + [null] + ptrs[i + 1:], good) == 1, i
    for i in (0, 1, 2, 3, 4, 5, 6, 8):                      # non-positive sizes
        for bad in (0, -1):
            assert call(ptrs, good[:i] + [bad] + good[i + 1:]) == 1, (i, bad)
    assert call(ptrs, good[:5] + [cap + 1] + good[6:]) == 1          # tables wider than the kernel's cap
    assert call(ptrs, good[:6] + [cap + 1] + good[7:]) == 1
    assert call(ptrs, good[:7] + [316, 585] + good[9:]) == 1         # source rows 316..900 of 900
    assert call(ptrs, good[:7] + [-1, 585] + good[9:]) == 1
    assert call(ptrs, good[:7] + [0, 901] + good[9:]) == 1
    assert call(ptrs, good[:2] + [4097] + good[3:]) == 1             # wider than the staged source row
    assert call(ptrs, good[:4] + [2049] + good[5:]) == 1             # wider than the staged output row
    assert call([ctypes.c_void_p(264)] + ptrs[1:], good) == 1        # output not 16-byte aligned
    assert h.simpb_preprocess_mid_pitch(704) == 2112 and h.simpb_preprocess_mid_pitch(1408) == 4224
    assert h.simpb_preprocess_mid_pitch(5) == 32 and h.simpb_preprocess_mid_pitch(0) == 0 and h.simpb_preprocess_mid_pitch(2049) == 0
