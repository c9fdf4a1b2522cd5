"""numpy witness of the ingest's YCbCr -> BGR conversion (simpb_amd/preprocess.py:yuv_coefficients, csrc/preprocess.hip), for
the YCbCr ingest tests. Plain int64 numpy, written apart from the product: the matrices are derived here from Kr / Kb.

One image is u8 [Hs * 3 / 2, Ws]: rows 0 .. Hs - 1 luma, rows Hs .. Hs * 3 / 2 - 1 interleaved chroma pairs, (Cb, Cr) for NV12
(vu_order = 0) and (Cr, Cb) for NV21 (vu_order = 1). Chroma sample (i, j) belongs to luma rows 2i, 2i + 1 and columns 2j,
2j + 1 (replicated). With 16 fractional bits,

    c = iy * (Y - yoff) + 2^15
    R = clip8((c + irv * (Cr - 128)) >> 16)
    G = clip8((c + igu * (Cb - 128) + igv * (Cr - 128)) >> 16)
    B = clip8((c + ibu * (Cb - 128)) >> 16)"""
import numpy as np

# standard: (Kr, Kb, full range)
STANDARDS = {"jfif": (0.299, 0.114, True), "bt601": (0.299, 0.114, False), "bt709": (0.2126, 0.0722, False)}


def matrix(standard):
    """float64 (yoff, y gain, Cr -> R, Cb -> G, Cr -> G, Cb -> B)."""
    kr, kb, full = STANDARDS[standard]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    return (0 if full else 16, ys, 2 * (1 - kr) * cs, -2 * kb * (1 - kb) / kg * cs, -2 * kr * (1 - kr) / kg * cs, 2 * (1 - kb) * cs)


def integer_matrix(standard):
    m = matrix(standard)
    return (m[0],) + tuple(int(np.floor(65536.0 * v + 0.5)) for v in m[1:])


def convert(y, cb, cr, standard):
    """The integer rule on arrays of equal shape -> (B, G, R) int64 arrays in 0..255."""
    yoff, iy, irv, igu, igv, ibu = integer_matrix(standard)
    y, cb, cr = (np.asarray(v).astype(np.int64) for v in (y, cb, cr))
    c = iy * (y - yoff) + (1 << 15)
    parts = (c + ibu * (cb - 128), c + igu * (cb - 128) + igv * (cr - 128), c + irv * (cr - 128))
    for v in parts + (c,):
        assert v.size == 0 or (np.abs(v).max() < 2 ** 31)
    return tuple(np.clip(v >> 16, 0, 255) for v in parts)


def exact(y, cb, cr, standard):
    """The float64 matrix, rounded to nearest and clamped -> (B, G, R)."""
    yoff, ys, rv, gu, gv, bu = matrix(standard)
    y, cb, cr = (np.asarray(v).astype(np.float64) for v in (y, cb, cr))
    c = ys * (y - yoff)
    parts = (c + bu * (cb - 128), c + gu * (cb - 128) + gv * (cr - 128), c + rv * (cr - 128))
    return tuple(np.clip(np.floor(v + 0.5), 0, 255).astype(np.int64) for v in parts)


def yuv420sp_to_bgr(frame, standard="jfif", vu_order=0):
    """u8 [..., Hs * 3 / 2, Ws] -> u8 [..., Hs, Ws, 3] (B, G, R)."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.shape[-2] % 3 == 0 and frame.shape[-1] % 2 == 0
    hs, ws = frame.shape[-2] * 2 // 3, frame.shape[-1]
    assert hs % 2 == 0
    luma = frame[..., :hs, :]
    pairs = frame[..., hs:, :].reshape(frame.shape[:-2] + (hs // 2, ws // 2, 2))
    cb, cr = pairs[..., 1 if vu_order else 0], pairs[..., 0 if vu_order else 1]
    up = lambda c: np.repeat(np.repeat(c, 2, axis=-2), 2, axis=-1)   # noqa: E731  (replication)
    return np.stack(convert(luma, up(cb), up(cr), standard), axis=-1).astype(np.uint8)


def bgr_to_nv12(frame_bgr, standard="jfif"):
    """u8 [..., Hs, Ws, 3] -> u8 [..., Hs * 3 / 2, Ws] NV12: the float forward transform with 2 x 2 chroma averaging. Only a
    way to make natural-looking inputs: nothing is asserted about it."""
    kr, kb, full = STANDARDS[standard]
    x = np.asarray(frame_bgr).astype(np.float32)    # (single precision is plenty for making inputs)
    hs, ws = x.shape[-3], x.shape[-2]
    assert hs % 2 == 0 and ws % 2 == 0
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    y = kr * r + (1 - kr - kb) * g + kb * b
    cb, cr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    pool = lambda c: c.reshape(c.shape[:-2] + (hs // 2, 2, ws // 2, 2)).mean(axis=(-3, -1))   # noqa: E731
    if full:
        y8, cb8, cr8 = y, pool(cb) + 128, pool(cr) + 128
    else:
        y8, cb8, cr8 = 16 + y * 219 / 255, 128 + pool(cb) * 224 / 255, 128 + pool(cr) * 224 / 255
    q = lambda v: np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)   # noqa: E731
    chroma = np.stack([q(cb8), q(cr8)], axis=-1).reshape(x.shape[:-3] + (hs // 2, ws))
    return np.ascontiguousarray(np.concatenate([q(y8), chroma], axis=-2))


def to_nv21(frame_nv12):
    """The same picture with the chroma pairs swapped."""
    f = np.array(frame_nv12, copy=True)
    hs = f.shape[-2] * 2 // 3
    f[..., hs:, 0::2], f[..., hs:, 1::2] = frame_nv12[..., hs:, 1::2], frame_nv12[..., hs:, 0::2]
    return f
