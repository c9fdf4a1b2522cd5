"""numpy restatement of the reference's fourth ingest step, `img.rotate(rotate)` (datasets/pipelines/augment.py:92,105):
`PIL.Image.rotate` with its defaults -- nearest neighbour, no expand, about the image centre, black outside -- on a u8
[h, w, 3] image. Pillow maps every output pixel back into the input by an affine matrix in 16.16 fixed point
(src/libImaging/Geometry.c, affine_fixed) and takes a transpose instead for 180 degrees, and for 90 / 270 degrees on a
square image. Written apart from simpb_amd/preprocess.py (which reduces a roll to six integers for the kernel): here the
image is rotated, whole arrays at a time, so that the product's integers are checked against a second statement of the
rule and both against Pillow and the reference's own function (tests/golden/roll.npz)."""
import math

import numpy as np


def fixed(v):
    """Pillow's FIX: a double as 16.16 fixed point, rounded half up."""
    return math.floor(v * 65536.0 + 0.5)


def affine(angle, w, h):
    """Image.rotate's inverse matrix (a, b, c, d, e, f) for `angle` in [0, 360): output (x, y) <- input (a x + b y + c, d x + e y + f)."""
    rad = -math.radians(angle)
    a, b = round(math.cos(rad), 15), round(math.sin(rad), 15)
    d, e = round(-math.sin(rad), 15), round(math.cos(rad), 15)
    cx, cy = w / 2, h / 2
    c = a * -cx + b * -cy + 0.0
    f = d * -cx + e * -cy + 0.0
    return a, b, c + cx, d, e, f + cy


def rotate(img, degrees):
    """u8 [h, w, C] -> u8 [h, w, C]: `Image.fromarray(img).rotate(degrees)`."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    angle = degrees % 360.0
    if angle == 0:
        return img.copy()
    if angle == 180:
        return np.ascontiguousarray(img[::-1, ::-1])
    if angle in (90, 270) and w == h:   # counter-clockwise quarter turns
        return np.ascontiguousarray(np.rot90(img, 1 if angle == 90 else 3))
    assert h <= 8192 and w <= 8192   # (beyond, a corner may leave Pillow's fixed-point range, and Pillow another path)
    a, b, c, d, e, f = affine(angle, w, h)
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    # the pixel centre (x + 0.5, y + 0.5) goes through the matrix: the halves are folded into the constant terms
    xin = (fixed(c + a * 0.5 + b * 0.5) + y * fixed(b) + x * fixed(a)) >> 16
    yin = (fixed(f + d * 0.5 + e * 0.5) + y * fixed(e) + x * fixed(d)) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def gather(img, six):
    """The kernel's rule driven by six integers (a0 .. a5), in numpy: output (x, y) <- input ((a2 + y a1 + x a0) >> 16,
    (a5 + y a4 + x a3) >> 16) where that lies inside the image, black elsewhere."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = (int(v) for v in six)
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    xin, yin = (a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out

