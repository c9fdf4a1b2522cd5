"""Host side of the camera frame ingest (csrc/preprocess.hip): the integer tables of the reference's test pipeline
(projects/configs/simpb_nus_r50_img_704x256.py:349-358) for one (source size, aug_config, img_norm_cfg).

`ResizeCropFlipImage._img_transform` (datasets/pipelines/augment.py:86-106) is PIL.Image.resize(resize_dims).crop(crop) and
an optional left-right flip; Pillow's default filter for an RGB image is bicubic (a = -0.5), antialiased, in 8-bit fixed
point. `coefficients` restates Pillow's precompute_coeffs / normalize_coeffs_8bpc (src/libImaging/Resample.c) in float64;
everything after it is integer, so the device result equals Pillow's byte for byte (tests/test_preprocess_host.py pins
the statement to Pillow and to the reference's own function). `NormalizeMultiviewImage` (transform_3d.py:438-466) delegates
to mmcv.imnormalize, which is not vendored: (x - mean) * (1 / std) in fp32 after the BGR -> RGB swap is restated from its
published behaviour and parity-unpinned. This module computes tables only; no pixel is resampled on the host.

Frames may also arrive as 4:2:0 semi-planar YCbCr (NV12 / NV21), the form hardware video and JPEG decoders deliver:
`yuv_coefficients` defines the integer conversion to the (B, G, R) bytes above that the horizontal pass applies while it
stages a row; everything behind it is the BGR route's own."""
import ctypes
import math

import numpy as np

PRECISION_BITS = 22   # Pillow: 32 - 8 - 2
# img_norm_cfg of the shipped configs (:320-322)
IMG_NORM_CFG = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


FRAME_FORMATS = ("bgr", "nv12", "nv21")
YUV_BITS = 16         # fractional bits of the YCbCr -> BGR coefficients
# standard -> (Kr, Kb, full range)
YUV_STANDARDS = {"jfif": (0.299, 0.114, True), "bt601": (0.299, 0.114, False), "bt709": (0.2126, 0.0722, False)}


def yuv_coefficients(standard="jfif"):
    """(yoff, iy, irv, igu, igv, ibu) of a YCbCr standard: each floor(2^16 * x + 0.5) of the float64 matrix entry, for

        c = iy * (Y - yoff) + 2^15
        R = clip8((c + irv * (Cr - 128)) >> 16)
        G = clip8((c + igu * (Cb - 128) + igv * (Cr - 128)) >> 16)
        B = clip8((c + ibu * (Cb - 128)) >> 16)                      (>> arithmetic, clip8 clamps to 0..255)

    "jfif": full range, Kr = 0.299, Kb = 0.114 (what a JPEG holds; the default). "bt601": limited range (luma 16..235, chroma
    16..240), the same Kr / Kb. "bt709": limited range, Kr = 0.2126, Kb = 0.0722."""
    if standard not in YUV_STANDARDS:
        raise ValueError(f"colour standard {standard!r}: one of {sorted(YUV_STANDARDS)}")
    kr, kb, full = YUV_STANDARDS[standard]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    entries = (ys, 2.0 * (1.0 - kr) * cs, -2.0 * kb * (1.0 - kb) / kg * cs, -2.0 * kr * (1.0 - kr) / kg * cs, 2.0 * (1.0 - kb) * cs)
    iy, irv, igu, igv, ibu = (int(math.floor(v * (1 << YUV_BITS) + 0.5)) for v in entries)
    yoff = 0 if full else 16
    # every partial sum stays far inside int32
    luma = max(abs(iy * (0 - yoff)), abs(iy * (255 - yoff))) + (1 << (YUV_BITS - 1))
    assert iy > 0 and luma + 128 * max(abs(irv), abs(ibu), abs(igu) + abs(igv)) < (1 << 31)
    return yoff, iy, irv, igu, igv, ibu


def _check_format(frame_format, colour):
    if frame_format not in FRAME_FORMATS:
        raise ValueError(f"frame format {frame_format!r}: one of {FRAME_FORMATS}")
    if colour not in YUV_STANDARDS:
        raise ValueError(f"colour standard {colour!r}: one of {sorted(YUV_STANDARDS)}")


def frame_shape(src_hw, frame_format="bgr"):
    """Trailing dimensions of one image of `src_hw` = (Hs, Ws): (Hs, Ws, 3) interleaved BGR, or (Hs * 3 / 2, Ws) for NV12 / NV21
    (Hs luma rows, then Hs / 2 rows of interleaved chroma pairs; row pitch Ws)."""
    hs, ws = int(src_hw[0]), int(src_hw[1])
    if frame_format == "bgr":
        return (hs, ws, 3)
    if hs % 2 or ws % 2:
        raise ValueError(f"{frame_format} frames have even sizes (one chroma pair per 2 x 2 luma samples), got {ws} x {hs}")
    return (hs * 3 // 2, ws)


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients(in_size, out_size):
    """(lo i32 [out], n i32 [out], k i32 [out, taps]) of one axis: output sample i = clip8((2^21 + sum_t src[lo[i] + t] *
    k[i, t]) >> 22), t < n[i]; entries past n[i] are zero. Equal sizes: Pillow does not resample that axis -> one tap of 1."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resize {in_size} -> {out_size}")
    one = 1 << PRECISION_BITS
    if in_size == out_size:
        return np.arange(out_size, dtype=np.int32), np.ones(out_size, np.int32), np.full((out_size, 1), one, np.int32)
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    rows, los = [], []
    for i in range(out_size):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = [_bicubic((j + lo - center + 0.5) * ss) for j in range(hi - lo)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        rows.append([int(v * one + 0.5) if v >= 0 else int(v * one - 0.5) for v in w])
        los.append(lo)
    taps = int(math.ceil(support)) * 2 + 1   # Pillow's ksize: the width of its coefficient rows
    assert taps >= max(len(r) for r in rows)
    k = np.zeros((out_size, taps), np.int64)
    for i, r in enumerate(rows):
        k[i, :len(r)] = r
    # every partial sum of a pass stays inside int32
    if not ((1 << (PRECISION_BITS - 1)) + 255 * np.abs(k).sum(1) < (1 << 31)).all():
        raise ValueError(f"resize {in_size} -> {out_size}: coefficient row overflows the int32 accumulator")
    return np.asarray(los, np.int32), np.asarray([len(r) for r in rows], np.int32), k.astype(np.int32)


def normalise_lut(img_norm_cfg=None):
    """f16 [3, 256]: lut[c][v] = f16((f32(v) - mean32[c]) * stdinv32[c]), stdinv32 = f32(1 / f64(std)): two separately
    rounded fp32 operations, then round-to-nearest-even to f16 -- what casting the host pipeline's fp32 image gives."""
    cfg = IMG_NORM_CFG if img_norm_cfg is None else img_norm_cfg
    mean = np.asarray(cfg["mean"], np.float64).astype(np.float32)
    stdinv = (1.0 / np.asarray(cfg["std"], np.float64)).astype(np.float32)
    if mean.shape != (3,) or stdinv.shape != (3,):
        raise ValueError("img_norm_cfg: three means and three stds")
    v = np.arange(256, dtype=np.float32)[None, :]
    diff = (v - mean[:, None]).astype(np.float32)
    return (diff * stdinv[:, None]).astype(np.float32).astype(np.float16)


def resolve_aug(src_hw, aug_config):
    """(resize_dims (W, H), crop (x0, y0, x1, y1), flip) of an aug_config dict for a source of src_hw = (Hs, Ws), with
    augment.py:88-92's defaults; ValueError / NotImplementedError for what the device path does not take."""
    hs, ws = int(src_hw[0]), int(src_hw[1])
    aug = aug_config or {}
    resize = aug.get("resize", 1)
    dims = aug.get("resize_dims")
    dims = (int(ws * resize), int(hs * resize)) if dims is None else (int(dims[0]), int(dims[1]))
    crop = tuple(int(v) for v in aug.get("crop", (0, 0) + dims))
    if aug.get("rotate", 0) != 0:
        raise NotImplementedError("rotate != 0 is a training augmentation (0 in test mode: nuscenes_dataset.py:217-230)")
    if hs <= 0 or ws <= 0 or dims[0] <= 0 or dims[1] <= 0:
        raise ValueError(f"source {ws} x {hs} -> resize_dims {dims}")
    if len(crop) != 4 or not (0 <= crop[0] < crop[2] <= dims[0] and 0 <= crop[1] < crop[3] <= dims[1]):
        raise ValueError(f"crop {crop} is not inside the resized image {dims[0]} x {dims[1]}")
    return dims, crop, bool(aug.get("flip", False))


def plan_key(src_hw, aug_config, frame_format="bgr", colour="jfif"):
    """What a ResamplePlan depends on: a frame whose key differs must not run on the plan's tables (nor a frame of another
    format or colour standard on the plan's kernel; the standard says nothing about BGR frames and is left out of their key)."""
    _check_format(frame_format, colour)
    dims, crop, flip = resolve_aug(src_hw, aug_config)
    return (int(src_hw[0]), int(src_hw[1]), dims, crop, flip, frame_format, colour if frame_format != "bgr" else None)


def _device(device):
    """torch.device with its index spelled out ("cuda" and "cuda:0" name the same tables)."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class ResamplePlan:
    """Tables of one ingest configuration; `upload(device)` makes them resident, `run(frames)` launches.

    frame_format "bgr": u8 [..., Hs, Ws, 3] interleaved pixels. "nv12" / "nv21": one image is a contiguous u8 [Hs * 3 / 2, Ws]:
    rows 0 .. Hs - 1 are luma, rows Hs .. Hs * 3 / 2 - 1 interleaved chroma pairs, (Cb, Cr) for nv12 and (Cr, Cb) for nv21;
    chroma sample (i, j) belongs to luma rows 2i, 2i + 1 and columns 2j, 2j + 1 and is replicated, not interpolated (the
    antialiased bicubic reduction behind it makes the choice of chroma up-sampler immaterial). Hs and Ws are even and the row
    pitch is Ws (a decoder's padded pitch is not taken). `colour` names the standard of `yuv_coefficients`. The converted
    pixel is staged as (B, G, R), so to_rgb, the table and the output mean what they mean for BGR frames: the output equals
    the BGR plan's on the converted frames bit for bit."""

    def __init__(self, src_hw, aug_config=None, img_norm_cfg=None, frame_format="bgr", colour="jfif"):
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        _check_format(frame_format, colour)
        self.frame_format, self.colour = frame_format, colour
        self.frame_shape = frame_shape(self.src_hw, frame_format)
        self.yuv = None if frame_format == "bgr" else yuv_coefficients(colour)
        self.resize_dims, self.crop, self.flip = resolve_aug(self.src_hw, aug_config)
        self.key = plan_key(self.src_hw, aug_config, frame_format, colour)
        cfg = IMG_NORM_CFG if img_norm_cfg is None else img_norm_cfg
        self.img_norm_cfg = dict(mean=list(cfg["mean"]), std=list(cfg["std"]), to_rgb=bool(cfg.get("to_rgb", True)))
        self.swap_rb = self.img_norm_cfg["to_rgb"]
        x0, y0, x1, y1 = self.crop
        self.out_hw = (y1 - y0, x1 - x0)
        xlo, xn, kx = coefficients(self.src_hw[1], self.resize_dims[0])
        ylo, yn, ky = coefficients(self.src_hw[0], self.resize_dims[1])
        # the kept columns' / rows' slice only; taps: the width of Pillow's coefficient rows (11 at 1600 -> 704, 7 at -> 1408)
        self.xlo, self.xn = xlo[x0:x1].copy(), xn[x0:x1].copy()
        self.ylo, self.yn = ylo[y0:y1].copy(), yn[y0:y1].copy()
        self.taps_x, self.taps_y = int(kx.shape[1]), int(ky.shape[1])
        self.kx = np.ascontiguousarray(kx[x0:x1])
        self.ky = np.ascontiguousarray(ky[y0:y1])
        # source rows the vertical pass of the kept rows reads: the horizontal pass runs for these alone
        self.src_row0 = int(self.ylo.min())
        self.src_rows = int((self.ylo + self.yn).max()) - self.src_row0
        self.lut = normalise_lut(self.img_norm_cfg)
        self._dev = None

    # ------------------------------------------------------------------ traffic the algorithm needs (tools/bench_preprocess.py)
    def bytes_per_image(self, mid_pitch):
        h, w = self.out_hw
        mid = self.src_rows * mid_pitch
        if self.yuv is None:
            source = self.src_rows * self.src_hw[1] * 3
        else:   # the needed luma rows and the distinct chroma rows under them (needed bytes: both luma rows of a pair stage it)
            last = self.src_row0 + self.src_rows - 1
            source = (self.src_rows + (last >> 1) - (self.src_row0 >> 1) + 1) * self.src_hw[1]
        return dict(source=source, mid_write=mid, mid_read=mid, out=h * w * 8)

    # ------------------------------------------------------------------ device
    def upload(self, device):
        import torch
        from . import _lib
        lib = _lib.lib()
        if self.taps_x > 64 or self.taps_y > 64 or self.src_hw[1] > 4096 or self.out_hw[1] > 2048:
            raise ValueError(f"ingest of {self.src_hw} -> {self.resize_dims} is outside the kernel's limits "
                             "(source width 4096, output width 2048, 64 taps)")
        device = _device(device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
        self._dev = dict(device=device, kx=t(self.kx), xlo=t(self.xlo), xn=t(self.xn), ky=t(self.ky), ylo=t(self.ylo),
                         yn=t(self.yn), lut=t(self.lut), pitch=int(lib.simpb_preprocess_mid_pitch(self.out_hw[1])), mid=None)
        return self

    def reserve(self, num_images, device):
        """Allocate the intermediate buffer for `num_images` now (a runner does this before any graph capture)."""
        import torch
        if self._dev is None or self._dev["device"] != _device(device):
            self.upload(device)
        d = self._dev
        if d["mid"] is None or d["mid"].numel() < num_images * self.src_rows * d["pitch"]:
            d["mid"] = torch.empty(num_images * self.src_rows * d["pitch"], dtype=torch.uint8, device=d["device"])
        return self

    def layout(self):
        """The frames `run` takes, in words (for error messages)."""
        hs, ws = self.src_hw
        if self.yuv is None:
            return f"u8 [..., {hs}, {ws}, 3] frames (interleaved BGR)"
        pair = "(Cb, Cr)" if self.frame_format == "nv12" else "(Cr, Cb)"
        return (f"u8 [..., {hs * 3 // 2}, {ws}] {self.frame_format} frames ({hs} luma rows, then {hs // 2} rows of interleaved {pair} "
                f"pairs, row pitch {ws}: a padded pitch is not taken)")

    def check_frames(self, frames):
        """ValueError unless `frames` is u8 with this plan's frame layout behind at least one leading dimension."""
        import torch
        k = len(self.frame_shape)
        if frames.dtype != torch.uint8 or frames.dim() <= k or tuple(frames.shape[-k:]) != self.frame_shape:
            raise ValueError(f"ingest takes {self.layout()}, got {frames.dtype} {tuple(frames.shape)}")

    def run(self, frames, out=None):
        """frames u8 [..., Hs, Ws, 3] (u8 [..., Hs * 3 / 2, Ws] for nv12 / nv21) on the device (contiguous) -> f16 [N, h, w, 4]
        (N = product of the leading dimensions), channel 3 = 0. Launches on the current stream; the intermediate buffer is
        allocated on first use and kept."""
        import torch
        from . import _lib
        hs, ws = self.src_hw
        self.check_frames(frames)
        if not frames.is_cuda:
            raise RuntimeError("simpb_amd operators run on the GPU only (got a CPU tensor); there is no CPU fallback")
        if not frames.is_contiguous():
            raise ValueError("ingest takes contiguous frames" + (" (interleaved pixels)" if self.yuv is None else ""))
        n = int(frames.numel() // int(np.prod(self.frame_shape)))
        h, w = self.out_hw
        if n == 0:
            raise ValueError("ingest of an empty batch")
        self.reserve(n, frames.device)
        d = self._dev
        if out is None:
            out = torch.empty(n, h, w, 4, dtype=torch.float16, device=frames.device)
        elif out.dtype != torch.float16 or tuple(out.shape) != (n, h, w, 4) or not out.is_contiguous():
            raise ValueError(f"ingest writes f16 [{n}, {h}, {w}, 4]")
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        args = (p(out), p(frames), p(d["mid"]), p(d["kx"]), p(d["xlo"]), p(d["xn"]), p(d["ky"]), p(d["ylo"]), p(d["yn"]), p(d["lut"]),
                n, hs, ws, h, w, self.taps_x, self.taps_y, self.src_row0, self.src_rows, int(self.flip), int(self.swap_rb))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.yuv is None:
            _lib.check(_lib.lib().simpb_preprocess_u8_nhwc4_f16(*args, stream), "simpb_preprocess_u8_nhwc4_f16")
        else:
            _lib.check(_lib.lib().simpb_preprocess_yuv420sp_nhwc4_f16(*args, int(self.frame_format == "nv21"), *self.yuv, stream),
                       "simpb_preprocess_yuv420sp_nhwc4_f16")
        return out
