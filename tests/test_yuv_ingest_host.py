"""CPU: the host side of the YCbCr (NV12 / NV21) ingest. The integer conversion (tests/yuv_ref.py, a witness written apart
from the product) against the float64 matrices and against Pillow over the whole 256^3 cube; the product's coefficients,
plan keys, frame layout and refusals (simpb_amd/preprocess.py); the C entry's argument checks, which run before any HIP call."""
import ctypes

import numpy as np
import pytest

from simpb_amd import preprocess as P
from tests import yuv_ref as Y

TABLE = {"jfif": (0, 65536, 91881, -22553, -46802, 116130),
         "bt601": (16, 76309, 104597, -25675, -53279, 132201),
         "bt709": (16, 76309, 117489, -13975, -34925, 138438)}


def cube_slices():
    """(Y [1, 1], Cb [256, 1], Cr [1, 256]) per luma value: the 256^3 cube in 256 slices."""
    cb, cr = np.arange(256)[:, None], np.arange(256)[None, :]
    for y in range(256):
        yield np.full((1, 1), y), cb, cr


def test_coefficients_are_the_documented_table():
    for standard, row in TABLE.items():
        assert P.yuv_coefficients(standard) == row
        assert Y.integer_matrix(standard) == row      # the witness derives the same integers by itself
    assert P.yuv_coefficients() == TABLE["jfif"]


@pytest.mark.parametrize("standard", sorted(TABLE))
def test_witness_against_float64_over_the_cube(standard):
    """Integer rule with 16 fractional bits against clip(floor(exact + 0.5)) of the float64 matrix: never more than 1 apart,
    and apart on at most 0.1 % of the cube's 3 x 2^24 channel values (0.029 % jfif, 0.017 % bt601 / bt709 when written)."""
    worst, differ = 0, 0
    for y, cb, cr in cube_slices():
        got, want = Y.convert(y, cb, cr, standard), Y.exact(y, cb, cr, standard)
        for g, w in zip(got, want):
            d = np.abs(np.broadcast_to(g, (256, 256)) - np.broadcast_to(w, (256, 256)))
            worst = max(worst, int(d.max()))
            differ += int((d != 0).sum())
    share = differ / (3 * 256 ** 3)
    print(f"{standard}: max |int - float64| = {worst}, differing share = {100 * share:.4f} %")
    assert worst <= 1
    assert share <= 0.001


def test_witness_against_pillow_jfif_over_the_cube():
    """A closeness check, not byte parity: Pillow's own YCbCr -> RGB tables carry 6 fractional bits, so it and the 16-bit rule
    differ by 1 on about a third of the cube; they never differ by more."""
    Image = pytest.importorskip("PIL.Image")
    worst = 0
    for y, cb, cr in cube_slices():
        ycc = np.stack(np.broadcast_arrays(np.broadcast_to(y, (256, 256)), cb, cr), -1).astype(np.uint8)
        rgb = np.asarray(Image.frombytes("YCbCr", (256, 256), ycc.tobytes()).convert("RGB")).astype(np.int64)
        b, g, r = Y.convert(y, cb, cr, "jfif")
        for ch, v in ((0, r), (1, g), (2, b)):
            worst = max(worst, int(np.abs(rgb[..., ch] - v).max()))
    print(f"jfif: max |witness - Pillow| = {worst}")
    assert worst <= 1


@pytest.mark.parametrize("vu_order", [0, 1])
def test_replication_layout(vu_order):
    """Chroma planes that are ramps: every luma pixel of a 2 x 2 block takes the block's own chroma sample, in both orders.
    Under jfif with Y = 128 and Cr = 128, B = clip8(128 + 1.772 (Cb - 128)) is strictly increasing in Cb over 80..172, and the
    same holds for R in Cr (1.402): each sample is recognised in the converted pixels."""
    hs, ws = 8, 12
    frame = np.full((hs * 3 // 2, ws), 128, np.uint8)
    i, j = np.meshgrid(np.arange(hs // 2), np.arange(ws // 2), indexing="ij")
    ramp = (80 + 4 * (i * (ws // 2) + j)).astype(np.uint8)        # 24 distinct values, 80..172: inside the unclamped range
    for which in ("cb", "cr"):
        f = frame.copy()
        col = (0 if which == "cb" else 1) ^ vu_order
        f[hs:, col::2] = ramp
        bgr = Y.yuv420sp_to_bgr(f, "jfif", vu_order).astype(np.int64)
        want = Y.convert(128, ramp if which == "cb" else 128, ramp if which == "cr" else 128, "jfif")[0 if which == "cb" else 2]
        got = bgr[..., 0 if which == "cb" else 2]
        assert len(np.unique(want)) == ramp.size
        for dy in (0, 1):
            for dx in (0, 1):
                assert np.array_equal(got[dy::2, dx::2], np.broadcast_to(want, ramp.shape)), (which, dy, dx)


def test_plan_keys_differ_by_format_and_standard():
    aug = dict(resize=0.5)
    keys = [P.plan_key((90, 160), aug)] + [P.plan_key((90, 160), aug, f, c) for f in ("nv12", "nv21") for c in sorted(TABLE)]
    assert len(set(keys)) == len(keys) == 7
    assert P.plan_key((90, 160), aug) == P.plan_key((90, 160), aug, "bgr", "jfif")
    for f in ("nv12", "nv21"):
        for c in sorted(TABLE):
            plan = P.ResamplePlan((90, 160), aug, None, f, c)
            assert plan.key == P.plan_key((90, 160), aug, f, c) and plan.key != P.ResamplePlan((90, 160), aug).key
            assert plan.yuv == TABLE[c] and plan.frame_shape == (135, 160)
    bgr = P.ResamplePlan((90, 160), aug)
    assert bgr.frame_format == "bgr" and bgr.yuv is None and bgr.frame_shape == (90, 160, 3)
    # the tables behind the conversion are the BGR plan's own
    nv = P.ResamplePlan((90, 160), aug, frame_format="nv12")
    assert np.array_equal(nv.kx, bgr.kx) and np.array_equal(nv.ky, bgr.ky) and (nv.src_row0, nv.src_rows) == (bgr.src_row0, bgr.src_rows)


def test_refusals_name_the_layout():
    torch = pytest.importorskip("torch")
    for hw in ((91, 160), (90, 161)):
        with pytest.raises(ValueError, match="even"):
            P.ResamplePlan(hw, dict(resize=0.5), frame_format="nv12")
        P.ResamplePlan(hw, dict(resize=0.5))    # (a BGR frame may be odd)
    with pytest.raises(ValueError, match="frame format"):
        P.ResamplePlan((90, 160), None, frame_format="i420")
    with pytest.raises(ValueError, match="colour standard"):
        P.ResamplePlan((90, 160), None, frame_format="nv12", colour="bt2020")
    with pytest.raises(ValueError, match="colour standard"):
        P.yuv_coefficients("smpte240m")
    with pytest.raises(ValueError):
        P.plan_key((90, 160), None, "nv12", "rec709")
    plan = P.ResamplePlan((90, 160), dict(resize=0.5), frame_format="nv21")
    for bad in (torch.zeros(1, 90, 160, 3, dtype=torch.uint8),        # the BGR layout
                torch.zeros(1, 135, 192, dtype=torch.uint8),          # a padded pitch
                torch.zeros(135, 160, dtype=torch.uint8),             # no leading dimension
                torch.zeros(1, 135, 160, dtype=torch.float32)):
        with pytest.raises(ValueError, match=r"135, 160\] nv21 frames \(90 luma rows, then 45 rows of interleaved \(Cr, Cb\) pairs, "
                                             r"row pitch 160: a padded pitch is not taken\)"):
            plan.run(bad)
    with pytest.raises(ValueError, match=r"90, 160, 3\] frames"):
        P.ResamplePlan((90, 160), dict(resize=0.5)).run(torch.zeros(1, 135, 160, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU only"):
        plan.run(torch.zeros(1, 135, 160, dtype=torch.uint8))         # right layout, host memory: no CPU route


def test_bytes_per_image():
    r50 = dict(resize=0.44, crop=(0, 140, 704, 396))
    bgr = P.ResamplePlan((900, 1600), r50)
    nv = P.ResamplePlan((900, 1600), r50, frame_format="nv12")
    a, b = bgr.bytes_per_image(2112), nv.bytes_per_image(2112)
    first, last = nv.src_row0, nv.src_row0 + nv.src_rows - 1
    chroma_rows = len({r >> 1 for r in range(first, last + 1)})
    assert a["source"] == bgr.src_rows * 1600 * 3
    assert b["source"] == nv.src_rows * 1600 + chroma_rows * 1600
    assert {k: v for k, v in a.items() if k != "source"} == {k: v for k, v in b.items() if k != "source"}
    # an odd first row and an even last one: both ends share their chroma row with a row that is not read
    odd = P.ResamplePlan((64, 96), dict(resize=1, crop=(0, 3, 96, 8)), frame_format="nv21")
    assert (odd.src_row0, odd.src_rows) == (3, 5)
    assert odd.bytes_per_image(288)["source"] == 5 * 96 + 3 * 96


def test_c_entry_refuses_bad_arguments_before_any_hip_call():
    """As tests/test_capi.py: validation precedes any HIP call, so it is checkable without a device."""
    from simpb_amd import _lib
    h = _lib.lib()
    fn = h.simpb_preprocess_yuv420sp_nhwc4_f16
    null, ok = ctypes.c_void_p(0), ctypes.c_void_p(64)
    ints = dict(num_images=1, src_height=90, src_width=160, out_height=45, out_width=80, taps_x=9, taps_y=9, src_row0=0, src_rows=90,
                flip=0, swap_rb=1, vu_order=0, yoff=0, iy=65536, irv=91881, igu=-22553, igv=-46802, ibu=116130)

    def call(ptrs=None, **changed):
        vals = dict(ints, **changed)
        return fn(*(ptrs or [ok] * 10), *vals.values(), null)

    for i in range(10):
        assert call([null if j == i else ok for j in range(10)]) == 1, i
    assert call(src_height=91, src_rows=91) == 1
    assert call(src_width=161) == 1
    assert call(vu_order=2) == 1 and call(vu_order=-1) == 1
    assert call(iy=0) == 1 and call(iy=-65536) == 1
    # what the BGR entry refuses is refused as well
    assert call(num_images=0) == 1 and call(src_width=4098) == 1 and call(out_width=2049) == 1 and call(taps_x=65) == 1
    assert call(src_row0=1) == 1 and call([ctypes.c_void_p(72)] + [ok] * 9) == 1
