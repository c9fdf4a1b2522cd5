"""numpy helpers of the surface ingest tests (padded decoder surfaces and P010; simpb_amd/preprocess.py:SurfaceLayout,
csrc/preprocess.hip). Written apart from the product: a layout is only read for its numbers (pitch, chroma_pitch,
chroma_offset, image_bytes, src_hw, frame_format), and the 10-bit colour rule is restated here from the witness's integers
(tests/yuv_ref.py), with two more fractional bits:

    c = iy (Y10 - 4 yoff) + 2^17
    R = clip8((c + irv (Cr10 - 512)) >> 18)
    G = clip8((c + igu (Cb10 - 512) + igv (Cr10 - 512)) >> 18)
    B = clip8((c + ibu (Cb10 - 512)) >> 18)

A tight frame is u8 [..., Hs, Ws, 3] (bgr), u8 [..., Hs * 3 / 2, Ws] (nv12 / nv21) or u16 [..., Hs * 3 / 2, Ws] (p010, sample =
word >> 6, stored little-endian); a surface is u8 [..., image_bytes]."""
import numpy as np

from tests import yuv_ref as Y


def _rows(layout):
    """(offset of row r's first byte, for every luma / BGR row and then every chroma row; sample bytes of a row)."""
    hs, ws = layout.src_hw
    if layout.frame_format == "bgr":
        return [r * layout.pitch for r in range(hs)], ws * 3
    sample = 2 if layout.frame_format == "p010" else 1
    offsets = [r * layout.pitch for r in range(hs)] + [layout.chroma_offset + i * layout.chroma_pitch for i in range(hs // 2)]
    return offsets, ws * sample


def _tight_bytes(tight_frame, layout):
    """The tight frame as u8 [..., rows, row bytes]."""
    f = np.asarray(tight_frame)
    if layout.frame_format == "bgr":
        assert f.dtype == np.uint8
        return f.reshape(f.shape[:-2] + (f.shape[-2] * 3,))
    if layout.frame_format == "p010":
        assert f.dtype == np.uint16
        return np.ascontiguousarray(f.astype("<u2")).view(np.uint8)
    assert f.dtype == np.uint8
    return f


def pack(tight_frame, layout, fill=0):
    """The tight frame placed into surfaces u8 [..., image_bytes] of `layout`. Every byte that is no sample is `fill`: a
    constant, or a numpy RandomState for random bytes."""
    rows = _tight_bytes(tight_frame, layout)
    offsets, row_bytes = _rows(layout)
    assert rows.shape[-2:] == (len(offsets), row_bytes), (rows.shape, len(offsets), row_bytes)
    shape = rows.shape[:-2] + (layout.image_bytes,)
    if isinstance(fill, np.random.RandomState):
        out = fill.randint(0, 256, shape).astype(np.uint8)
    else:
        out = np.full(shape, fill, np.uint8)
    for r, off in enumerate(offsets):
        out[..., off:off + row_bytes] = rows[..., r, :]
    return out


def unpack(surface, layout):
    """The tight frame of surfaces u8 [..., image_bytes]: `pack`'s inverse."""
    surface = np.asarray(surface)
    assert surface.dtype == np.uint8 and surface.shape[-1] == layout.image_bytes
    offsets, row_bytes = _rows(layout)
    rows = np.stack([surface[..., off:off + row_bytes] for off in offsets], axis=-2)
    hs, ws = layout.src_hw
    if layout.frame_format == "bgr":
        return rows.reshape(rows.shape[:-1] + (ws, 3))
    if layout.frame_format == "p010":
        return np.ascontiguousarray(rows).view("<u2").astype(np.uint16)
    return rows


def sample_mask(layout):
    """bool [image_bytes]: True where a byte belongs to a sample."""
    mask = np.zeros(layout.image_bytes, bool)
    offsets, row_bytes = _rows(layout)
    for off in offsets:
        assert not mask[off:off + row_bytes].any(), "rows overlap"
        mask[off:off + row_bytes] = True
    return mask


def to_p010(nv12_frame, low_bits=0):
    """An 8-bit NV12 frame lifted to P010 words u16 [..., Hs * 3 / 2, Ws]: v << 8, the low six bits `low_bits` (a constant below
    64, or a numpy RandomState for random ones)."""
    f = np.asarray(nv12_frame)
    assert f.dtype == np.uint8
    if isinstance(low_bits, np.random.RandomState):
        low = low_bits.randint(0, 64, f.shape).astype(np.uint16)
    else:
        assert 0 <= int(low_bits) < 64
        low = np.uint16(low_bits)
    return (f.astype(np.uint16) << 8) | low


def convert10(y, cb, cr, standard):
    """The 10-bit integer rule on arrays of 10-bit samples -> (B, G, R) int64 arrays in 0..255, and the largest |partial sum|."""
    yoff, iy, irv, igu, igv, ibu = Y.integer_matrix(standard)
    y, cb, cr = (np.asarray(v).astype(np.int64) for v in (y, cb, cr))
    c = iy * (y - 4 * yoff) + (1 << 17)
    cb, cr = cb - 512, cr - 512
    parts = (c + ibu * cb, c + igu * cb + igv * cr, c + irv * cr)
    steps = parts + (c, c + igu * cb, ibu * cb, igu * cb, igv * cr, irv * cr)
    bound = max(int(np.abs(v).max()) for v in steps if v.size)
    assert bound < 2 ** 31
    return tuple(np.clip(v >> 18, 0, 255) for v in parts), bound


def exact10(y, cb, cr, standard):
    """The float64 matrix on 10-bit limited-range samples, rounded to 8 bits: luma (Y10 - 64) * 255 / 876, chroma (C10 - 512) *
    255 / 896 -> (B, G, R)."""
    kr, kb, full = Y.STANDARDS[standard]
    assert not full
    kg = 1.0 - kr - kb
    y, cb, cr = (np.asarray(v).astype(np.float64) for v in (y, cb, cr))
    c = (y - 64.0) * 255.0 / 876.0
    u, v = (cb - 512.0) * 255.0 / 896.0, (cr - 512.0) * 255.0 / 896.0
    parts = (c + 2 * (1 - kb) * u, c - 2 * kb * (1 - kb) / kg * u - 2 * kr * (1 - kr) / kg * v, c + 2 * (1 - kr) * v)
    return tuple(np.clip(np.floor(p + 0.5), 0, 255).astype(np.int64) for p in parts)


def p010_to_bgr(surface, layout, standard):
    """P010 surfaces u8 [..., image_bytes] -> u8 [..., Hs, Ws, 3] (B, G, R) by the 10-bit rule; chroma sample (i, j) belongs to
    luma rows 2i, 2i + 1 and columns 2j, 2j + 1 (replicated)."""
    assert layout.frame_format == "p010"
    words = unpack(surface, layout) >> 6
    hs, ws = layout.src_hw
    luma = words[..., :hs, :]
    pairs = words[..., hs:, :].reshape(words.shape[:-2] + (hs // 2, ws // 2, 2))
    up = lambda c: np.repeat(np.repeat(c, 2, axis=-2), 2, axis=-1)   # noqa: E731
    return np.stack(convert10(luma, up(pairs[..., 0]), up(pairs[..., 1]), standard)[0], axis=-1).astype(np.uint8)
