"""numpy restatement of the reference's test-time image pipeline, for the ingest tests: Pillow's 8-bit bicubic resize
(src/libImaging/Resample.c, what `PIL.Image.resize(dims)` does for an RGB image), crop, left-right flip
(datasets/pipelines/augment.py:86-106), then NormalizeMultiviewImage (transform_3d.py:438-466). Written apart from
simpb_amd/preprocess.py on purpose (vectorised numpy there is none to share: that module makes tables only, this one
resamples pixels), so that the product's tables are checked against a second statement of the rule and both against Pillow."""
import math

import numpy as np

BITS = 22


def cubic(x):
    x = -x if x < 0 else x
    if x < 1:
        return (1.5 * x - 2.5) * x * x + 1
    if x < 2:
        return (((x - 5) * x + 8) * x - 4) * -0.5
    return 0.0


def axis_table(n_in, n_out):
    """[(first source index, [integer coefficients])] per output sample."""
    scale = n_in / n_out
    fs = scale if scale > 1 else 1.0
    support = 2.0 * fs
    inv = 1.0 / fs
    table = []
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = int(c - support + 0.5)
        lo = 0 if lo < 0 else lo
        hi = int(c + support + 0.5)
        hi = n_in if hi > n_in else hi
        w = [cubic((j + lo - c + 0.5) * inv) for j in range(hi - lo)]
        s = 0.0
        for v in w:
            s += v
        w = [v / s for v in w] if s != 0 else w
        table.append((lo, [math.trunc(v * (1 << BITS) + (0.5 if v >= 0 else -0.5)) for v in w]))
    return table


def resample_axis(img, n_out, axis):
    """One pass over u8 `img` along `axis` (0: rows, 1: columns); equal sizes: untouched, as in Pillow."""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for i, (lo, k) in enumerate(axis_table(n_in, n_out)):
        acc = np.full(src.shape[1:], 1 << (BITS - 1), np.int64)
        for t, c in enumerate(k):
            acc += src[lo + t] * c
        assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31
        out[i] = np.clip(acc >> BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize(img, dims):
    """u8 [H, W, 3] -> u8 [dims[1], dims[0], 3]: horizontal pass, u8, vertical pass."""
    return resample_axis(resample_axis(img, dims[0], 1), dims[1], 0)


def img_transform(img, aug):
    """ResizeCropFlipImage._img_transform's image for rotate = 0, as u8 [h, w, 3]."""
    hs, ws = img.shape[:2]
    r = aug.get("resize", 1)
    dims = tuple(aug["resize_dims"]) if aug.get("resize_dims") is not None else (int(ws * r), int(hs * r))
    x0, y0, x1, y1 = aug.get("crop", (0, 0) + tuple(dims))
    out = resize(img, dims)[y0:y1, x0:x1]
    return np.ascontiguousarray(out[:, ::-1] if aug.get("flip", False) else out)


def normalise(img_u8, mean, std, to_rgb=True):
    """NormalizeMultiviewImage on one u8 [h, w, 3] image -> f32 [h, w, 3]: channel swap, minus mean, times 1 / std (fp32)."""
    x = img_u8.astype(np.float32)
    if to_rgb:
        x = x[..., ::-1]
    m = np.asarray(mean, np.float64).astype(np.float32)
    si = (1.0 / np.asarray(std, np.float64)).astype(np.float32)
    return ((x - m).astype(np.float32) * si).astype(np.float32)


def pipeline_nchw(frames_u8, aug, norm):
    """u8 [..., Hs, Ws, 3] -> f32 [..., 3, h, w]: the tensor the fp32 entry points take."""
    lead = frames_u8.shape[:-3]
    flat = frames_u8.reshape((-1,) + frames_u8.shape[-3:])
    out = np.stack([normalise(img_transform(f, aug), norm["mean"], norm["std"], norm.get("to_rgb", True)).transpose(2, 0, 1) for f in flat])
    return np.ascontiguousarray(out.reshape(lead + out.shape[1:]))


def nhwc4_f16(frames_u8, aug, norm):
    """u8 [..., Hs, Ws, 3] -> f16 [N, h, w, 4], channel 3 = 0: what the device ingest must produce."""
    x = pipeline_nchw(frames_u8, aug, norm)
    x = x.reshape((-1,) + x.shape[-3:]).transpose(0, 2, 3, 1).astype(np.float16)
    return np.concatenate([x, np.zeros(x.shape[:3] + (1,), np.float16)], axis=-1)
