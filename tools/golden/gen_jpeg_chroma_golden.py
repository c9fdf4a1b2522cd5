"""Writes tests/golden/jpeg_chroma.npz: what libjpeg (through Pillow) makes of four small JPEG files, for the tests of the
ingest's JPEG-decoder planes (tests/test_chroma_host.py, tests/test_gpu_chroma.py). The data comes from Pillow alone; no file of
the reference is read.

Per size (H x W: 2 x 2, 6 x 10, 18 x 34, 32 x 48) a noisy picture is saved by Pillow as a JPEG with 4:2:0 and with 4:4:4 sampling,
and per file the fixture holds
    {name}_y, _cb, _cr   the file's NATIVE planes: luma [H, W]; chroma [H / 2, W / 2] at 4:2:0, [H, W] at 4:4:4
    {name}_rgb           Pillow's RGB decode of the same file, u8 [H, W, 3]
with name = f"s{subsampling}_{H}x{W}". The native chroma of a 4:2:0 file is taken with Image.draft("YCbCr", (W / 2, H / 2)): at half
scale libjpeg widens the chroma IDCT instead of upsampling, so the Cb / Cr channels of that decode are the file's own chroma
samples. Luma, and all three planes of a 4:4:4 file, come from the full-scale YCbCr decode (no upsampling there).

The seeds are chosen (`python tools/golden/gen_jpeg_chroma_golden.py --search`) so that every picture's decode holds a pixel whose
(Cb, Cr), after libjpeg's upsampling, is one of the 59 pairs at which the Kr / Kb-derived constant -22553 and libjpeg's -22554
give a different G: the fixture then tells colour "jfif" from colour "jpeg".

The bytes depend on the JPEG library: they regenerate identically where PIL.features.check_feature("libjpeg_turbo") holds
(written with Pillow 12.2). Arrays only.

    python tools/golden/gen_jpeg_chroma_golden.py
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_chroma.npz")
SIZES = ((2, 2), (6, 10), (18, 34), (32, 48))     # (H, W)
SUBSAMPLINGS = (2, 0)                              # Pillow's codes: 2 = 4:2:0, 0 = 4:4:4
QUALITY = 95
SEEDS = {(2, 2, 2): 1999, (2, 2, 0): 47, (6, 10, 2): 9, (6, 10, 0): 54, (18, 34, 2): 44, (18, 34, 0): 1, (32, 48, 2): 11, (32, 48, 0): 1}


def disagreeing_pairs():
    """bool [256, 256] over (Cb, Cr): G by -22553 differs from G by -22554 (the luma term is a multiple of 2^16 and drops out)."""
    cb, cr = np.meshgrid(np.arange(256, dtype=np.int64) - 128, np.arange(256, dtype=np.int64) - 128, indexing="ij")
    return ((32768 - 22553 * cb - 46802 * cr) >> 16) != ((32768 - 22554 * cb - 46802 * cr) >> 16)


def picture(seed, h, w):
    """u8 [h, w, 3] RGB: strong, saturated noise (the chroma planes then span most of their range)."""
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


def encode(rgb, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=QUALITY, subsampling=subsampling)
    return buf.getvalue()


def decode(data, mode=None, size=None):
    """Pillow's decode of a JPEG: RGB at full scale, or with `mode` / `size` through Image.draft."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if mode is not None:
        im.draft(mode, size)
        assert im.mode == mode, (im.mode, mode)
    return np.asarray(im).copy()


def planes_and_rgb(data, h, w, subsampling):
    """(y, cb, cr, rgb) of one file."""
    full = decode(data, "YCbCr", (w, h))
    assert full.shape == (h, w, 3)
    if subsampling == 0:
        cb, cr = full[..., 1], full[..., 2]
    else:
        half = decode(data, "YCbCr", (w // 2, h // 2))
        assert half.shape == (h // 2, w // 2, 3), half.shape
        cb, cr = half[..., 1], half[..., 2]
    rgb = decode(data)
    assert rgb.shape == (h, w, 3)
    return full[..., 0].copy(), cb.copy(), cr.copy(), rgb


def upsampled_chroma(data, h, w):
    """The (Cb, Cr) libjpeg converts: the chroma channels of the full-scale YCbCr decode."""
    full = decode(data, "YCbCr", (w, h))
    return full[..., 1], full[..., 2]


def holds_a_disagreeing_pair(data, h, w):
    cb, cr = upsampled_chroma(data, h, w)
    return bool(disagreeing_pairs()[cb, cr].any())


def arrays():
    out = {}
    for h, w in SIZES:
        for sub in SUBSAMPLINGS:
            data = encode(picture(SEEDS[h, w, sub], h, w), sub)
            assert holds_a_disagreeing_pair(data, h, w), (h, w, sub)
            name = f"s{sub}_{h}x{w}"
            for key, value in zip(("y", "cb", "cr", "rgb"), planes_and_rgb(data, h, w, sub)):
                out[f"{name}_{key}"] = np.ascontiguousarray(value, np.uint8)
    return out


def search():
    for (h, w, sub) in SEEDS:
        for seed in range(1, 100000):
            if holds_a_disagreeing_pair(encode(picture(seed, h, w), sub), h, w):
                print(f"({h}, {w}, {sub}): {seed},")
                break
        else:
            print(f"({h}, {w}, {sub}): none found")


def main():
    if "--search" in sys.argv:
        return search()
    # an .npz with a fixed time stamp on every member (np.savez stamps the clock): the file regenerates byte for byte
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for name, value in arrays().items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
