"""numpy helpers of the plane ingest tests (planar 4:2:0, packed 4:2:2 and the RGB-order family; simpb_amd/preprocess.py,
csrc/preprocess.hip: simpb_preprocess_planes_nhwc4_f16). Written apart from the product: a layout is only read for its numbers
(pitch, chroma_pitch, chroma_offset, chroma2_offset, image_bytes, src_hw, frame_format), and the colour rule is the witness's
(tests/yuv_ref.py: convert), with replicated chroma.

A tight frame is
    yuv420p / yvu420p   u8 [..., Hs * 3 / 2, Ws]: Hs luma rows, then Hs / 2 * Ws / 2 bytes of Cb (yvu420p: Cr) and as many of
                        the other plane, dense (a chroma plane's rows are Ws / 2 bytes: two of them fill one row of the array)
    yuyv / uyvy         u8 [..., Hs, Ws, 2]: groups of (Y0, Cb, Y1, Cr) / (Cb, Y0, Cr, Y1)
    rgb                 u8 [..., Hs, Ws, 3], R first
    bgra / rgba         u8 [..., Hs, Ws, 4], byte 3 anything
and the older formats' are those of tests/surface_ref.py, whose pack / unpack / sample_mask these functions fall back on. A
surface is u8 [..., image_bytes]."""
import numpy as np

from tests import surface_ref as S
from tests import yuv_ref as Y

PLANAR = ("yuv420p", "yvu420p")
PACKED_422 = ("yuyv", "uyvy")
PIXEL_BYTES = {"yuyv": 2, "uyvy": 2, "rgb": 3, "bgra": 4, "rgba": 4}
NEW = PLANAR + tuple(PIXEL_BYTES)


# ----------------------------------------------------------------------------------------------------------- tight frames
def planes(frame, fmt):
    """(luma [..., Hs, Ws], cb [..., Hs / 2, Ws / 2], cr [..., Hs / 2, Ws / 2]) of a tight planar frame."""
    frame = np.asarray(frame)
    assert fmt in PLANAR and frame.dtype == np.uint8 and frame.shape[-2] % 3 == 0 and frame.shape[-1] % 2 == 0
    hs, ws = frame.shape[-2] * 2 // 3, frame.shape[-1]
    assert hs % 2 == 0
    lead = frame.shape[:-2]
    flat = frame.reshape(lead + (-1,))
    n = hs * ws
    first = flat[..., n:n + n // 4].reshape(lead + (hs // 2, ws // 2))
    second = flat[..., n + n // 4:].reshape(lead + (hs // 2, ws // 2))
    cb, cr = (first, second) if fmt == "yuv420p" else (second, first)
    return flat[..., :n].reshape(lead + (hs, ws)), cb, cr


def from_planes(luma, cb, cr, fmt):
    """The tight planar frame u8 [..., Hs * 3 / 2, Ws] of three planes: `planes`' inverse."""
    luma, cb, cr = (np.asarray(v, np.uint8) for v in (luma, cb, cr))
    hs, ws = luma.shape[-2:]
    assert cb.shape == cr.shape == luma.shape[:-2] + (hs // 2, ws // 2) and hs % 2 == 0 and ws % 2 == 0
    lead = luma.shape[:-2]
    order = (cb, cr) if fmt == "yuv420p" else (cr, cb)
    flat = np.concatenate([luma.reshape(lead + (-1,))] + [c.reshape(lead + (-1,)) for c in order], axis=-1)
    return np.ascontiguousarray(flat.reshape(lead + (hs * 3 // 2, ws)))


def planar_from_nv12(nv12_frame, fmt):
    """An NV12 frame u8 [..., Hs * 3 / 2, Ws] -> the same picture as a tight yuv420p / yvu420p frame."""
    f = np.asarray(nv12_frame)
    hs = f.shape[-2] * 2 // 3
    return from_planes(f[..., :hs, :], f[..., hs:, 0::2], f[..., hs:, 1::2], fmt)


def nv12_from_planar(frame, fmt):
    """A tight planar frame re-interleaved into NV12 u8 [..., Hs * 3 / 2, Ws]."""
    luma, cb, cr = planes(frame, fmt)
    pairs = np.stack([cb, cr], axis=-1).reshape(cb.shape[:-1] + (cb.shape[-1] * 2,))
    return np.ascontiguousarray(np.concatenate([luma, pairs], axis=-2))


def packed_422(luma, cb, cr, fmt):
    """luma u8 [..., Hs, Ws], cb / cr u8 [..., Hs, Ws / 2] (a chroma pair per row and column pair) -> u8 [..., Hs, Ws, 2]."""
    luma, cb, cr = (np.asarray(v, np.uint8) for v in (luma, cb, cr))
    hs, ws = luma.shape[-2:]
    assert fmt in PACKED_422 and ws % 2 == 0 and cb.shape == cr.shape == luma.shape[:-1] + (ws // 2,)
    out = np.zeros(luma.shape + (2,), np.uint8)
    y, c = (0, 1) if fmt == "yuyv" else (1, 0)
    out[..., y] = luma
    out[..., 0::2, c] = cb
    out[..., 1::2, c] = cr
    return out


def swap_422(frame):
    """A yuyv frame as uyvy and the other way round: the two bytes of every pixel exchanged."""
    return np.ascontiguousarray(np.asarray(frame)[..., ::-1])


def from_bgr(bgr, fmt, alpha=0):
    """u8 [..., Hs, Ws, 3] (B, G, R) -> the rgb / bgra / rgba frame of the same picture; alpha: a constant or a RandomState."""
    bgr = np.asarray(bgr, np.uint8)
    if fmt == "rgb":
        return np.ascontiguousarray(bgr[..., ::-1])
    assert fmt in ("bgra", "rgba")
    if isinstance(alpha, np.random.RandomState):
        a = alpha.randint(0, 256, bgr.shape[:-1] + (1,)).astype(np.uint8)
    else:
        a = np.full(bgr.shape[:-1] + (1,), alpha, np.uint8)
    return np.ascontiguousarray(np.concatenate([bgr if fmt == "bgra" else bgr[..., ::-1], a], axis=-1))


def to_bgr(frame, fmt, standard="jfif"):
    """A tight frame of a new format -> u8 [..., Hs, Ws, 3] (B, G, R): the integer rule of yuv_ref.convert with replicated chroma
    for the YCbCr formats (4:2:0: a sample covers rows 2i, 2i + 1 and columns 2j, 2j + 1; 4:2:2: columns 2j, 2j + 1 of its own
    row), a byte permutation for the others."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8
    if fmt in PLANAR:
        luma, cb, cr = planes(frame, fmt)
        up = lambda c: np.repeat(np.repeat(c, 2, axis=-2), 2, axis=-1)   # noqa: E731
        return np.stack(Y.convert(luma, up(cb), up(cr), standard), axis=-1).astype(np.uint8)
    if fmt in PACKED_422:
        assert frame.shape[-1] == 2 and frame.shape[-2] % 2 == 0
        y, c = (0, 1) if fmt == "yuyv" else (1, 0)
        up = lambda v: np.repeat(v, 2, axis=-1)   # noqa: E731
        return np.stack(Y.convert(frame[..., y], up(frame[..., 0::2, c]), up(frame[..., 1::2, c]), standard), axis=-1).astype(np.uint8)
    if fmt == "rgb":
        assert frame.shape[-1] == 3
        return np.ascontiguousarray(frame[..., ::-1])
    assert fmt in ("bgra", "rgba") and frame.shape[-1] == 4
    return np.ascontiguousarray(frame[..., :3] if fmt == "bgra" else frame[..., 2::-1])


# --------------------------------------------------------------------------------------------------------------- surfaces
def _rows(layout):
    """[(offset of a row's first byte, its sample bytes)] in the order of the tight frame's bytes."""
    hs, ws = layout.src_hw
    fmt = layout.frame_format
    if fmt in PIXEL_BYTES:
        return [(r * layout.pitch, ws * PIXEL_BYTES[fmt]) for r in range(hs)]
    assert fmt in PLANAR
    cb = [(layout.chroma_offset + i * layout.chroma_pitch, ws // 2) for i in range(hs // 2)]
    cr = [(layout.chroma2_offset + i * layout.chroma_pitch, ws // 2) for i in range(hs // 2)]
    return [(r * layout.pitch, ws) for r in range(hs)] + (cb + cr if fmt == "yuv420p" else cr + cb)


def pack(tight_frame, layout, fill=0):
    """The tight frame placed into surfaces u8 [..., image_bytes] of `layout`. Every byte that is no sample is `fill`: a
    constant, or a numpy RandomState for random bytes."""
    if layout.frame_format not in NEW:
        return S.pack(tight_frame, layout, fill)
    f = np.asarray(tight_frame)
    assert f.dtype == np.uint8
    k = 2 if layout.frame_format in PLANAR else 3
    lead = f.shape[:-k]
    flat = f.reshape(lead + (-1,))
    rows = _rows(layout)
    assert flat.shape[-1] == sum(n for _, n in rows), (f.shape, layout.frame_format)
    shape = lead + (layout.image_bytes,)
    if isinstance(fill, np.random.RandomState):
        out = fill.randint(0, 256, shape).astype(np.uint8)
    else:
        out = np.full(shape, fill, np.uint8)
    at = 0
    for off, n in rows:
        out[..., off:off + n] = flat[..., at:at + n]
        at += n
    return out


def unpack(surface, layout):
    """The tight frame of surfaces u8 [..., image_bytes]: `pack`'s inverse."""
    if layout.frame_format not in NEW:
        return S.unpack(surface, layout)
    surface = np.asarray(surface)
    assert surface.dtype == np.uint8 and surface.shape[-1] == layout.image_bytes
    flat = np.concatenate([surface[..., off:off + n] for off, n in _rows(layout)], axis=-1)
    hs, ws = layout.src_hw
    fmt = layout.frame_format
    shape = (hs * 3 // 2, ws) if fmt in PLANAR else (hs, ws, PIXEL_BYTES[fmt])
    return np.ascontiguousarray(flat.reshape(surface.shape[:-1] + shape))


def sample_mask(layout):
    """bool [image_bytes]: True where a byte belongs to a sample (the alpha bytes of a 4-byte pixel are read: they count)."""
    if layout.frame_format not in NEW:
        return S.sample_mask(layout)
    mask = np.zeros(layout.image_bytes, bool)
    for off, n in _rows(layout):
        assert not mask[off:off + n].any(), "rows overlap"
        mask[off:off + n] = True
    return mask
