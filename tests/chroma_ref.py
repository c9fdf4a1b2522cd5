"""numpy witness of the ingest's JPEG-decoder planes (simpb_amd/preprocess.py: chroma="jpeg", colour="jpeg", "yuv444p";
csrc/preprocess.hip: fancy_pair), for tests/test_chroma_host.py and tests/test_gpu_chroma.py. Written apart from the product:
whole-plane numpy, libjpeg's constants typed in here, the other colour standards from tests/yuv_ref.py.

THE RULE. C is a native (subsampled) chroma plane [Hc, Wc], u8; the arithmetic is int32.
4:2:0, libjpeg's h2v2_fancy_upsample, for luma row r and column x:
    i = r >> 1,  j = x >> 1
    near = C[i],  far = C[clamp(i + (r odd ? +1 : -1), 0, Hc - 1)],  s[j] = 3 * near[j] + far[j]
    x even:  (3 * s[j] + s[max(j - 1, 0)]      + 8) >> 4
    x odd:   (3 * s[j] + s[min(j + 1, Wc - 1)] + 7) >> 4
4:2:2, libjpeg's h2v1_fancy_upsample, per row, c that row's chroma:
    x even:  (3 * c[j] + c[max(j - 1, 0)]      + 1) >> 2
    x odd:   (3 * c[j] + c[min(j + 1, Wc - 1)] + 2) >> 2
Colour "jpeg": the integer rule of tests/yuv_ref.py with libjpeg's own constants (jdcolor.c: FIX(1.40200), FIX(0.34414),
FIX(0.71414), FIX(1.77200)), every pixel with its own Cb / Cr.

`fancy` was checked against Pillow's decoder (libjpeg-turbo) on the native planes of JPEG files; tests/test_chroma_host.py
repeats that on tests/golden/jpeg_chroma.npz. `h2v1` is stated from libjpeg's published algorithm: libjpeg hands out no native
planes of a 4:2:2 file, so there is nothing to pin it to."""
import numpy as np

from tests import planes_ref as L
from tests import yuv_ref as Y

JPEG = (0, 65536, 91881, -22554, -46802, 116130)      # (yoff, iy, irv, igu, igv, ibu)
INTERPOLATED = ("nv12", "nv21", "yuv420p", "yvu420p", "yuyv", "uyvy")


def fancy(c):
    """h2v2: a native chroma plane [..., h, w] -> [..., 2h, 2w]."""
    c = np.asarray(c).astype(np.int32)
    up = np.concatenate([c[..., :1, :], c[..., :-1, :]], axis=-2)
    dn = np.concatenate([c[..., 1:, :], c[..., -1:, :]], axis=-2)
    out = np.zeros(c.shape[:-2] + (2 * c.shape[-2], 2 * c.shape[-1]), np.int32)
    for par, far in ((0, up), (1, dn)):
        s = 3 * c + far
        left = np.concatenate([s[..., :1], s[..., :-1]], axis=-1)
        right = np.concatenate([s[..., 1:], s[..., -1:]], axis=-1)
        out[..., par::2, 0::2] = (3 * s + left + 8) >> 4
        out[..., par::2, 1::2] = (3 * s + right + 7) >> 4
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def h2v1(c):
    """h2v1: chroma rows [..., h, w] -> [..., h, 2w]."""
    c = np.asarray(c).astype(np.int32)
    left = np.concatenate([c[..., :1], c[..., :-1]], axis=-1)
    right = np.concatenate([c[..., 1:], c[..., -1:]], axis=-1)
    out = np.zeros(c.shape[:-1] + (2 * c.shape[-1],), np.int32)
    out[..., 0::2] = (3 * c + left + 1) >> 2
    out[..., 1::2] = (3 * c + right + 2) >> 2
    return out.astype(np.uint8)


def integers(colour):
    return JPEG if colour == "jpeg" else Y.integer_matrix(colour)


def convert(y, cb, cr, colour="jpeg"):
    """Arrays of equal shape, a Cb / Cr per pixel -> u8 [..., 3] (B, G, R) by the integer rule with `colour`'s constants."""
    yoff, iy, irv, igu, igv, ibu = integers(colour)
    y, cb, cr = (np.asarray(v).astype(np.int64) for v in (y, cb, cr))
    c = iy * (y - yoff) + (1 << 15)
    parts = (c + ibu * (cb - 128), c + igu * (cb - 128) + igv * (cr - 128), c + irv * (cr - 128))
    assert all(np.abs(v).max() < 2 ** 31 for v in parts)
    return np.stack([np.clip(v >> 16, 0, 255) for v in parts], axis=-1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ tight frames
def planes444(frame):
    """(luma, cb, cr), each [..., Hs, Ws], of a tight yuv444p frame u8 [..., Hs * 3, Ws]."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.shape[-2] % 3 == 0
    hs = frame.shape[-2] // 3
    return frame[..., :hs, :], frame[..., hs:2 * hs, :], frame[..., 2 * hs:, :]


def frame444(luma, cb, cr):
    return np.ascontiguousarray(np.concatenate([np.asarray(v, np.uint8) for v in (luma, cb, cr)], axis=-2))


def nv12_frame(luma, cb, cr):
    """Native planes (luma [..., Hs, Ws], cb / cr [..., Hs / 2, Ws / 2]) -> the tight NV12 frame u8 [..., Hs * 3 / 2, Ws]."""
    return L.nv12_from_planar(L.from_planes(luma, cb, cr, "yuv420p"), "yuv420p")


def samples(frame, fmt):
    """(luma [..., Hs, Ws], native cb, native cr) of a tight frame: [..., Hs / 2, Ws / 2] for 4:2:0, [..., Hs, Ws / 2] for 4:2:2."""
    frame = np.asarray(frame)
    if fmt in ("nv12", "nv21"):
        hs = frame.shape[-2] * 2 // 3
        a, b = frame[..., hs:, 0::2], frame[..., hs:, 1::2]
        return (frame[..., :hs, :],) + ((a, b) if fmt == "nv12" else (b, a))
    if fmt in L.PLANAR:
        return L.planes(frame, fmt)
    assert fmt in L.PACKED_422
    y, c = (0, 1) if fmt == "yuyv" else (1, 0)
    return frame[..., y], frame[..., 0::2, c], frame[..., 1::2, c]


def to_bgr(frame, fmt, colour="jpeg"):
    """A tight frame -> u8 [..., Hs, Ws, 3] (B, G, R): interpolated chroma for the six subsampled formats, the samples as they
    are for "yuv444p"."""
    if fmt == "yuv444p":
        return convert(*planes444(frame), colour)
    assert fmt in INTERPOLATED
    luma, cb, cr = samples(frame, fmt)
    up = h2v1 if fmt in L.PACKED_422 else fancy
    return convert(luma, up(cb), up(cr), colour)


# ---------------------------------------------------------------------------------------------------------------- surfaces
def pack(tight_frame, layout, fill=0):
    """planes_ref.pack, and "yuv444p" beside it: the tight frame placed into surfaces u8 [..., image_bytes]; every byte that is
    no sample is `fill` (a constant, or a RandomState)."""
    if layout.frame_format != "yuv444p":
        return L.pack(tight_frame, layout, fill)
    f = np.asarray(tight_frame)
    hs, ws = layout.src_hw
    assert f.dtype == np.uint8 and f.shape[-2:] == (hs * 3, ws)
    shape = f.shape[:-2] + (layout.image_bytes,)
    out = fill.randint(0, 256, shape).astype(np.uint8) if isinstance(fill, np.random.RandomState) else np.full(shape, fill, np.uint8)
    starts = [(0, layout.pitch), (layout.chroma_offset, layout.chroma_pitch), (layout.chroma2_offset, layout.chroma_pitch)]
    for plane, (at, pitch) in enumerate(starts):
        for r in range(hs):
            out[..., at + r * pitch:at + r * pitch + ws] = f[..., plane * hs + r, :]
    return out
