"""Writes tests/golden/roll.npz: the reference's own `ResizeCropFlipImage._img_transform`
(projects/mmdet3d_plugin/datasets/pipelines/augment.py:86-132, read from the reference tree at generation time, never
copied) with `rotate != 0`: the six small cases of gen_preprocess_golden.py at six angles each, and one square crop at 90
and 270 degrees (where Pillow takes a transpose). Per case the image it returns, as u8, and the 4 x 4 matrix it returns;
the source images once each. Arrays and settings only. The reference function is loaded the way gen_preprocess_golden.py loads it; Pillow does the work,
exactly as in the reference. Runs where the reference tree and Pillow are present; the tests read only the .npz.

    python tools/golden/gen_roll_golden.py [reference root]
"""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_preprocess_golden import REF_ROOT, ROOT, cases, load_reference_transform, smooth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "roll.npz")
ANGLES = (180, 90, 7.5, -3.25, 45, 0.2)


def roll_cases():
    """(image, resize, crop or None, flip, rotate)"""
    for img, resize, crop, flip in list(cases()):
        for angle in ANGLES:
            yield img, resize, crop, flip, angle
    square = smooth(np.random.RandomState(20241), 70, 110)
    for angle in (90, 270):
        yield square, 0.5, (6, 2, 36, 32), True, angle   # a 30 x 30 crop


def main():
    transform = load_reference_transform(sys.argv[1] if len(sys.argv) > 1 else REF_ROOT)
    arrays, sources = {}, {}
    count = 0
    for i, (img, resize, crop, flip, angle) in enumerate(roll_cases()):
        aug = dict(resize=resize, flip=flip, rotate=angle)
        if crop is not None:
            aug["crop"] = crop
        out, mat = transform(img.copy(), aug)
        out = np.asarray(out)
        assert out.dtype == np.float32 and np.array_equal(out, np.round(out)) and out.min() >= 0 and out.max() <= 255
        key = [k for k, v in sources.items() if v is img]   # every source image is stored once
        if not key:
            key = [len(sources)]
            sources[key[0]] = img
            arrays[f"img{key[0]}"] = img
        arrays[f"case{i}_source"] = np.int64(key[0])
        arrays[f"case{i}_resize"] = np.float64(resize)
        arrays[f"case{i}_crop"] = np.asarray(crop if crop is not None else (), np.int64)
        arrays[f"case{i}_flip"] = np.bool_(flip)
        arrays[f"case{i}_rotate"] = np.float64(angle)
        arrays[f"case{i}_out"] = out.astype(np.uint8)
        arrays[f"case{i}_matrix"] = np.asarray(mat, np.float64)
        count += 1
    arrays["num_cases"] = np.int64(count)
    # an .npz with a fixed time stamp on every member (np.savez stamps the clock): the file regenerates byte for byte
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes,", count, "cases")


if __name__ == "__main__":
    main()
