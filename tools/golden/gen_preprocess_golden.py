"""Writes tests/golden/preprocess.npz: the reference's own `ResizeCropFlipImage._img_transform`
(projects/mmdet3d_plugin/datasets/pipelines/augment.py:86-106, read from the reference tree at generation time, never
copied) on a few small seeded uint8 images. Arrays and settings only.

The reference module imports cv2, mmcv and mmdet.datasets.builder, none of which that function uses: inert stand-ins are
installed here (empty modules, a PIPELINES whose register_module() hands the class back unchanged). Pillow does the
work, exactly as in the reference. Runs where the reference tree and Pillow are present; the tests read only the .npz.

    python tools/golden/gen_preprocess_golden.py [reference root]
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_shim import REF_ROOT  # noqa: E402  (where the reference tree lies in the build container; nothing else of the shim is used)
OUT = os.path.join(ROOT, "tests", "golden", "preprocess.npz")


def load_reference_transform(ref_root):
    class _Pipelines:
        @staticmethod
        def register_module(*args, **kwargs):
            return lambda cls: cls

    for name in ("cv2", "mmcv", "mmdet", "mmdet.datasets", "mmdet.datasets.builder"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["mmdet.datasets.builder"].PIPELINES = _Pipelines
    path = os.path.join(ref_root, "projects", "mmdet3d_plugin", "datasets", "pipelines", "augment.py")
    spec = importlib.util.spec_from_file_location("_ref_augment", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ResizeCropFlipImage()._img_transform


def smooth(rng, h, w):
    """Low-frequency colour waves: something for the resampler to interpolate, and it compresses."""
    y = np.arange(h, dtype=np.float64)[:, None, None] / h
    x = np.arange(w, dtype=np.float64)[None, :, None] / w
    fx, fy, ph = rng.uniform(0.5, 3.0, 3), rng.uniform(0.5, 3.0, 3), rng.uniform(0, 6.28, 3)
    return np.clip(127.5 + 140.0 * np.sin(6.283185307 * (fx * x + fy * y) + ph), 0, 255).astype(np.uint8)


def cases():
    rng = np.random.RandomState(20240)
    # (image, resize, crop or None (the reference's default: the whole resized image), flip)
    yield rng.randint(0, 256, (61, 97, 3)).astype(np.uint8), 0.44, (3, 5, 40, 24), False        # noise: both clamps, all the time
    yield smooth(rng, 89, 161), 0.47, (7, 11, 73, 40), True                                     # odd sizes, offsets on both axes
    yield smooth(rng, 90, 160), 0.44, None, False                                               # the shipped ratio, default crop
    yield smooth(rng, 60, 100), 1, (4, 6, 96, 54), True                                         # no resampling: crop + flip alone
    yield smooth(rng, 75, 120), 1.3, (1, 2, 150, 90), False                                     # enlargement (support 2.0)
    yield smooth(rng, 64, 150), 0.5, (0, 9, 75, 32), True                                       # offset on one axis only


def main():
    transform = load_reference_transform(sys.argv[1] if len(sys.argv) > 1 else REF_ROOT)
    arrays = {}
    count = 0
    for i, (img, resize, crop, flip) in enumerate(cases()):
        aug = dict(resize=resize, flip=flip, rotate=0)
        if crop is not None:
            aug["crop"] = crop
        out, _ = transform(img.copy(), aug)
        out = np.asarray(out)
        assert out.dtype == np.float32 and np.array_equal(out, np.round(out)) and out.min() >= 0 and out.max() <= 255
        arrays[f"case{i}_img"] = img
        arrays[f"case{i}_resize"] = np.float64(resize)
        arrays[f"case{i}_crop"] = np.asarray(crop if crop is not None else (), np.int64)
        arrays[f"case{i}_flip"] = np.bool_(flip)
        arrays[f"case{i}_out"] = out.astype(np.uint8)
        count += 1
    arrays["num_cases"] = np.int64(count)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", count, "cases")


if __name__ == "__main__":
    main()
