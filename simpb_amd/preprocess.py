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
stages a row; everything behind it is the BGR route's own. `SurfaceLayout` describes how a decoder lays such an image out
in memory (padded row pitch, aligned plane height, the chroma plane's own pitch and offset, tail padding) and adds P010, the
10-bit form of NV12 (`p010_coefficients`); `ResamplePlan.run_surfaces` takes one allocation per image.

A ResamplePlan describes all its images as one layout. `CameraSource` / `RigPlan` describe a rig whose cameras differ (source
size, format, layout, resize, crop, flip): per camera the tables of that camera's own ResamplePlan, one output size, two
launches for the whole rig, and the per-camera numbers the 2D record and the intrinsics need (`box2d_table`, `image_transforms`).

Frames of the other producers in a vehicle are taken as they lie as well: a software decoder's planar 4:2:0 ("yuv420p" = I420,
"yvu420p" = YV12), the packed 4:2:2 of a camera that reaches the host without a codec ("yuyv", "uyvy"), and the RGB-order and
4-byte pixels of loaders, ISPs and compositors ("rgb", "bgra", "rgba"). The YCbCr ones follow `yuv_coefficients` with
replicated chroma, the others are a byte permutation: no new arithmetic, and the output equals the BGR plan's on the
host-converted frames bit for bit.

A camera's mount roll -- the reference function's fourth step, `img.rotate(rotate)` (augment.py:92,105) -- is `roll=` of a
ResamplePlan or CameraSource: `roll_integers` reduces it to the six 16.16 fixed-point integers of Pillow's nearest-neighbour affine
map, which the vertical pass applies as a gather; the aug_config's own `rotate` stays refused (0 in the reference's test mode).

The reference's images are JPEG files decoded by libjpeg at its defaults. A caller who hands over the decoder's native planes gets
libjpeg's bytes with `chroma="jpeg"` (the subsampled chroma interpolated by libjpeg's "fancy" upsampling, in integers, inside the
horizontal pass), `colour="jpeg"` (libjpeg's own four colour constants, `YUV_INTEGERS`) and "yuv444p" (the three full planes of a
4:4:4 file). 4:2:0, 4:4:4 and the constants are pinned to libjpeg-turbo through Pillow; the 4:2:2 rule is stated only."""
import ctypes
import math

import numpy as np

PRECISION_BITS = 22   # Pillow: 32 - 8 - 2
# img_norm_cfg of the shipped configs (:320-322)
IMG_NORM_CFG = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


FRAME_FORMATS = ("bgr", "nv12", "nv21", "p010", "yuv420p", "yvu420p", "yuyv", "uyvy", "rgb", "bgra", "rgba")
# SIMPB_SURFACE_* of include/simpb_hip.h (the two planar names differ in their default plane order alone)
SURFACE_FORMAT = {"bgr": 0, "nv12": 1, "nv21": 2, "p010": 3, "yuv420p": 8, "yvu420p": 8, "yuyv": 9, "uyvy": 10, "rgb": 11, "bgra": 12,
                  "rgba": 13}
SEMI_PLANAR = ("nv12", "nv21", "p010")      # a luma plane and one plane of interleaved chroma pairs
PLANAR = ("yuv420p", "yvu420p")             # a luma plane, a Cb plane and a Cr plane
PACKED_422 = ("yuyv", "uyvy")               # one plane: (Y0, Cb, Y1, Cr) / (Cb, Y0, Cr, Y1)
PIXEL_BYTES = {"bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4, "yuyv": 2, "uyvy": 2}   # the one-plane formats
RGB_ORDER = ("bgr", "rgb", "bgra", "rgba")  # no YCbCr conversion: the colour standard says nothing about them
YUV_BITS = 16         # fractional bits of the YCbCr -> BGR coefficients
# standard -> (Kr, Kb, full range)
YUV_STANDARDS = {"jfif": (0.299, 0.114, True), "bt601": (0.299, 0.114, False), "bt709": (0.2126, 0.0722, False)}
# A colour given as its six integers (yoff, iy, irv, igu, igv, ibu), not derived from Kr / Kb. "jpeg": libjpeg's own YCbCr -> RGB
# tables (jdcolor.c), FIX(1.40200) = 91881, -FIX(0.34414) = -22554, -FIX(0.71414) = -46802, FIX(1.77200) = 116130 with FIX(x) =
# int(x * 65536 + 0.5) of the four rounded decimals. "jfif" rounds the exact 0.344136... to -22553, and G then differs by one at
# 59 of the 65 536 (Cb, Cr) pairs; "jfif" keeps its constants and its bytes.
YUV_INTEGERS = {"jpeg": (0, 65536, 91881, -22554, -46802, 116130)}
COLOURS = tuple(sorted(YUV_STANDARDS)) + tuple(sorted(YUV_INTEGERS))
# The frame formats of FRAME_FORMATS have subsampled chroma or none. "yuv444p" is the one with full-resolution chroma: three
# planes of Hs rows of Ws bytes, what a 4:4:4 JPEG decodes to. Every place that takes a frame format takes it.
FULL_CHROMA = ("yuv444p",)
ALL_FORMATS = FRAME_FORMATS + FULL_CHROMA
SURFACE_FORMAT["yuv444p"] = 16
# chroma="replicate" | "jpeg": how the subsampled chroma of a frame becomes a Cb / Cr per pixel. "replicate": sample (i, j)
# covers its 2 x 2 (4:2:2: 1 x 2) pixels. "jpeg": centre-sited samples, interpolated by libjpeg's "fancy" upsampling (its default
# for a JPEG file; include/simpb_hip.h: SIMPB_SURFACE_CHROMA_JPEG has the rule).
CHROMA_MODES = ("replicate", "jpeg")
CHROMA_JPEG_FLAG = 0x100              # SIMPB_SURFACE_CHROMA_JPEG
CHROMA_JPEG_FORMATS = ("nv12", "nv21", "yuv420p", "yvu420p", "yuyv", "uyvy")   # 8-bit samples, subsampled chroma


def yuv_coefficients(standard="jfif"):
    """(yoff, iy, irv, igu, igv, ibu) of a YCbCr standard: each floor(2^16 * x + 0.5) of the float64 matrix entry, for

        c = iy * (Y - yoff) + 2^15
        R = clip8((c + irv * (Cr - 128)) >> 16)
        G = clip8((c + igu * (Cb - 128) + igv * (Cr - 128)) >> 16)
        B = clip8((c + ibu * (Cb - 128)) >> 16)                      (>> arithmetic, clip8 clamps to 0..255)

    "jfif": full range, Kr = 0.299, Kb = 0.114 (what a JPEG holds; the default). "bt601": limited range (luma 16..235, chroma
    16..240), the same Kr / Kb. "bt709": limited range, Kr = 0.2126, Kb = 0.0722. "jpeg": full range, libjpeg's own four
    constants as they stand (YUV_INTEGERS), for the bytes its decoder gives."""
    if standard in YUV_INTEGERS:
        return YUV_INTEGERS[standard]
    if standard not in YUV_STANDARDS:
        raise ValueError(f"colour standard {standard!r}: one of {list(COLOURS)}")
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


def p010_coefficients(standard):
    """The six integers of `yuv_coefficients(standard)` for 10-bit samples (P010: sample = u16 word >> 6), used with two more
    fractional bits:

        c = iy * (Y10 - 4 * yoff) + 2^17
        R = clip8((c + irv * (Cr10 - 512)) >> 18)
        G = clip8((c + igu * (Cb10 - 512) + igv * (Cr10 - 512)) >> 18)
        B = clip8((c + ibu * (Cb10 - 512)) >> 18)

    An 8-bit sample stored as v << 8 (10-bit value 4 v) gives the 8-bit rule's byte, since (4 A) >> 18 == A >> 16. Limited
    range only ("bt601", "bt709"): JFIF is the 8-bit JPEG convention, and full-range 10-bit video scales by 1023, not by
    4 x 255."""
    if standard in YUV_INTEGERS:
        raise ValueError(f"colour {standard!r} is libjpeg's table for the 8-bit samples of a JPEG: p010 frames take 'bt601' or 'bt709'")
    if standard not in YUV_STANDARDS:
        raise ValueError(f"colour standard {standard!r}: one of {list(COLOURS)}")
    if YUV_STANDARDS[standard][2]:
        raise ValueError(f"colour standard {standard!r} is the full-range 8-bit JPEG convention: p010 frames take 'bt601' or 'bt709'")
    yoff, iy, irv, igu, igv, ibu = yuv_coefficients(standard)
    # every partial sum stays far inside int32 (below 1.45e8 for both standards)
    luma = max(abs(iy * (0 - 4 * yoff)), abs(iy * (1023 - 4 * yoff))) + (1 << (YUV_BITS + 1))
    assert luma + 512 * max(abs(irv), abs(ibu), abs(igu) + abs(igv)) < 145_000_000 < (1 << 31)
    return yoff, iy, irv, igu, igv, ibu


def _unknown_format(frame_format):
    return ValueError(f"frame format {frame_format!r}: one of {ALL_FORMATS} (planar I420 is 'yuv420p', YV12 is 'yvu420p')")


def _check_format(frame_format, colour, chroma="replicate"):
    if frame_format not in ALL_FORMATS:
        raise _unknown_format(frame_format)
    if colour not in COLOURS:
        raise ValueError(f"colour standard {colour!r}: one of {list(COLOURS)}")
    if frame_format == "p010":
        p010_coefficients(colour)   # (refuses "jfif" and "jpeg")
    if chroma not in CHROMA_MODES:
        raise ValueError(f"chroma={chroma!r}: one of {CHROMA_MODES}")
    if chroma == "jpeg" and frame_format not in CHROMA_JPEG_FORMATS:
        why = ("its samples are 10-bit: libjpeg's rule is stated for the 8-bit planes of a JPEG" if frame_format == "p010"
               else "every pixel has its own chroma sample already" if frame_format in FULL_CHROMA
               else "it has no chroma planes")
        raise ValueError(f"chroma='jpeg' interpolates subsampled 8-bit chroma (one of {CHROMA_JPEG_FORMATS}): a {frame_format} frame "
                         f"does not take it, {why}")


def format_code(frame_format, chroma="replicate"):
    """The `format` argument of the C entry points: SIMPB_SURFACE_* of include/simpb_hip.h, | SIMPB_SURFACE_CHROMA_JPEG."""
    return SURFACE_FORMAT[frame_format] | (CHROMA_JPEG_FLAG if chroma == "jpeg" else 0)


def frame_shape(src_hw, frame_format="bgr"):
    """Trailing dimensions of one tightly packed image of `src_hw` = (Hs, Ws): (Hs, Ws, 3) interleaved BGR, or (Hs * 3 / 2, Ws) for
    NV12 / NV21 (Hs luma rows, then Hs / 2 rows of interleaved chroma pairs; row pitch Ws), or (Hs * 3 / 2, Ws * 2) for P010 (the
    bytes of u16 little-endian samples in the NV12 arrangement). "yuv420p" / "yvu420p": (Hs * 3 / 2, Ws) as NV12 -- the same
    bytes count, so a caller's buffers carry over: Hs luma rows, then the Cb (yvu420p: Cr) plane of Hs / 2 rows of Ws / 2 bytes,
    then the other one. "yuyv" / "uyvy": (Hs, Ws, 2). "rgb": (Hs, Ws, 3). "bgra" / "rgba": (Hs, Ws, 4). "yuv444p": (Hs * 3, Ws), the
    luma, Cb and Cr planes of Hs rows each, any size."""
    hs, ws = int(src_hw[0]), int(src_hw[1])
    if frame_format in FULL_CHROMA:
        return (hs * 3, ws)
    if frame_format in PIXEL_BYTES:
        if frame_format in PACKED_422 and ws % 2:
            raise ValueError(f"{frame_format} frames have an even width (one chroma pair per two luma samples), got {ws} x {hs}")
        return (hs, ws, PIXEL_BYTES[frame_format])
    if hs % 2 or ws % 2:
        raise ValueError(f"{frame_format} frames have even sizes (one chroma pair per 2 x 2 luma samples), got {ws} x {hs}")
    return (hs * 3 // 2, ws * (2 if frame_format == "p010" else 1))


class SurfaceLayout:
    """Where the samples of one image lie in a decoder's surface; the same for all images of a plan or runner.

    frame_format "bgr": one plane of Hs rows, 3 bytes per pixel. "nv12" / "nv21" / "p010": a luma plane of Hs rows, 1 byte per
    sample (2 for p010), and a chroma plane of Hs / 2 rows of interleaved pairs of the same row width. "yuv420p" / "yvu420p": a
    luma plane of Hs rows and two chroma planes of Hs / 2 rows of Ws / 2 bytes each. "yuyv" / "uyvy" (2 bytes per pixel), "rgb"
    (3), "bgra" / "rgba" (4): one plane, like "bgr". "yuv444p": a luma plane of Hs rows and two chroma planes of Hs rows of Ws
    bytes each, with the fields of "yuv420p" (chroma_pitch defaults to pitch, Cb lies first).
      pitch          bytes from one luma (packed) row to the next; at least the row's sample bytes (the default)
      luma_rows      the plane height the decoder allocated, >= Hs (default Hs)
      chroma_pitch   bytes from one chroma row to the next (default: pitch; planar: pitch // 2, shared by both chroma planes)
      chroma_offset  bytes from the image's first byte to chroma row 0 (default: luma_rows * pitch); planar: to row 0 of the
                     Cb plane, whichever name the format has
      chroma2_offset planar only: bytes to row 0 of the Cr plane. The two planar names differ in these two defaults alone:
                     "yuv420p" has Cb at luma_rows * pitch and Cr behind Cb's Hs / 2 rows, "yvu420p" Cr first and Cb behind it
      image_bytes    the extent of one image and the stride between the images of a contiguous batch (default: the end of the
                     last chroma / packed row; larger = tail padding)
    ValueError for rows or planes that overlap, a sample outside image_bytes, and odd offsets of 16-bit samples.
    `.tight`: every field has its default (for bgr / nv12 / nv21 the form a ResamplePlan without a layout takes). `.key`:
    what enters `plan_key` (None when tight)."""

    def __init__(self, src_hw, frame_format, pitch=None, luma_rows=None, chroma_pitch=None, chroma_offset=None, image_bytes=None,
                 chroma2_offset=None):
        if frame_format not in ALL_FORMATS:
            raise _unknown_format(frame_format)
        hs, ws = int(src_hw[0]), int(src_hw[1])
        if hs <= 0 or ws <= 0:
            raise ValueError(f"source {ws} x {hs}")
        self.src_hw, self.frame_format = (hs, ws), frame_format
        self.tight = all(v is None for v in (pitch, luma_rows, chroma_pitch, chroma_offset, image_bytes, chroma2_offset))
        self.sample_bytes = 2 if frame_format == "p010" else 1
        self.row_bytes = ws * PIXEL_BYTES.get(frame_format, self.sample_bytes)   # the samples of a luma (packed) row
        self.chroma_row_bytes = 0 if frame_format in PIXEL_BYTES else ws // 2 if frame_format in PLANAR else self.row_bytes
        self.chroma_rows = 0 if frame_format in PIXEL_BYTES else hs if frame_format in FULL_CHROMA else hs // 2
        self.pitch = self.row_bytes if pitch is None else int(pitch)
        self.chroma2_offset = 0
        if frame_format in PIXEL_BYTES:
            given = [n for n, v in (("luma_rows", luma_rows), ("chroma_pitch", chroma_pitch), ("chroma_offset", chroma_offset),
                                    ("chroma2_offset", chroma2_offset)) if v is not None]
            if given:
                raise ValueError(f"a {frame_format} surface is one plane: {', '.join(given)} must not be given")
            frame_shape((hs, ws), frame_format)   # (an even width for 4:2:2)
            self.luma_rows, self.chroma_pitch, self.chroma_offset = hs, 0, 0
            self.sample_end = (hs - 1) * self.pitch + self.row_bytes
        elif frame_format in SEMI_PLANAR:
            if chroma2_offset is not None:
                raise ValueError(f"a {frame_format} surface has one chroma plane of interleaved pairs: chroma2_offset must not be given")
            frame_shape((hs, ws), frame_format)   # (even sizes)
            self.luma_rows = hs if luma_rows is None else int(luma_rows)
            self.chroma_pitch = self.pitch if chroma_pitch is None else int(chroma_pitch)
            self.chroma_offset = self.luma_rows * self.pitch if chroma_offset is None else int(chroma_offset)
            self.sample_end = self.chroma_offset + (hs // 2 - 1) * self.chroma_pitch + self.row_bytes
        else:
            frame_shape((hs, ws), frame_format)   # (even sizes)
            self.luma_rows = hs if luma_rows is None else int(luma_rows)
            full = frame_format in FULL_CHROMA
            if chroma_pitch is None and self.pitch % 2 and not full:
                raise ValueError(f"{frame_format} surface of {ws} x {hs}: the default chroma_pitch is pitch // 2 and the pitch "
                                 f"{self.pitch} is odd: give chroma_pitch")
            self.chroma_pitch = (self.pitch if full else self.pitch // 2) if chroma_pitch is None else int(chroma_pitch)
            first, plane = self.luma_rows * self.pitch, self.chroma_rows * self.chroma_pitch
            cb, cr = (first + plane, first) if frame_format == "yvu420p" else (first, first + plane)
            self.chroma_offset = cb if chroma_offset is None else int(chroma_offset)
            self.chroma2_offset = cr if chroma2_offset is None else int(chroma2_offset)
            self.sample_end = (max(self.chroma_offset, self.chroma2_offset) + (self.chroma_rows - 1) * self.chroma_pitch
                               + self.chroma_row_bytes)
        self.image_bytes = self.sample_end if image_bytes is None else int(image_bytes)
        self._check()
        self.key = None if self.tight else (self.pitch, self.luma_rows, self.chroma_pitch, self.chroma_offset, self.image_bytes)
        if self.key is not None and frame_format in PLANAR + FULL_CHROMA:
            self.key += (self.chroma2_offset,)

    def _check(self):
        hs, ws = self.src_hw
        what = self.describe()
        if self.pitch < self.row_bytes:
            raise ValueError(f"{what}: rows overlap (a row holds {self.row_bytes} sample bytes, the pitch is {self.pitch})")
        if self.frame_format not in PIXEL_BYTES:
            if self.luma_rows < hs:
                raise ValueError(f"{what}: luma_rows {self.luma_rows} is below the {hs} rows of the picture")
            if self.chroma_pitch < self.chroma_row_bytes:
                raise ValueError(f"{what}: chroma rows overlap (a row holds {self.chroma_row_bytes} sample bytes, the chroma pitch is "
                                 f"{self.chroma_pitch})")
            luma_end = (hs - 1) * self.pitch + self.row_bytes
            if self.chroma_offset < luma_end:
                raise ValueError(f"{what}: planes overlap (the luma samples end at byte {luma_end}, the chroma plane starts at "
                                 f"{self.chroma_offset})")
            if self.frame_format in PLANAR + FULL_CHROMA:
                if self.chroma2_offset < luma_end:
                    raise ValueError(f"{what}: planes overlap (the luma samples end at byte {luma_end}, the Cr plane starts at "
                                     f"{self.chroma2_offset})")
                span = (self.chroma_rows - 1) * self.chroma_pitch + self.chroma_row_bytes
                if self.chroma_offset < self.chroma2_offset + span and self.chroma2_offset < self.chroma_offset + span:
                    raise ValueError(f"{what}: planes overlap (the Cb samples span bytes {self.chroma_offset} .. "
                                     f"{self.chroma_offset + span}, the Cr samples {self.chroma2_offset} .. {self.chroma2_offset + span})")
            if self.frame_format == "p010" and (self.pitch % 2 or self.chroma_pitch % 2 or self.chroma_offset % 2):
                raise ValueError(f"{what}: p010 samples are 16-bit words: pitch, chroma_pitch and chroma_offset must be even")
        if self.image_bytes < self.sample_end:
            raise ValueError(f"{what}: the last sample ends at byte {self.sample_end}, outside image_bytes {self.image_bytes}")
        if self.frame_format == "p010" and self.image_bytes % 2:
            raise ValueError(f"{what}: p010 samples are 16-bit words: image_bytes must be even")
        if max(self.pitch, self.chroma_pitch) > (1 << 30) or self.image_bytes > (1 << 40):
            raise ValueError(f"{what}: outside the kernel's limits (pitch 2^30, image 2^40 bytes)")

    PIXELS = {"bgr": "interleaved BGR", "rgb": "interleaved RGB", "bgra": "4-byte BGRA pixels", "rgba": "4-byte RGBA pixels",
              "yuyv": "packed 4:2:2, groups of (Y0, Cb, Y1, Cr)", "uyvy": "packed 4:2:2, groups of (Cb, Y0, Cr, Y1)"}

    def describe(self):
        """The layout in words (for error messages)."""
        hs, ws = self.src_hw
        if self.frame_format in PIXEL_BYTES:
            return f"{self.frame_format} surface of {ws} x {hs} ({self.PIXELS[self.frame_format]}, row pitch {self.pitch})"
        if self.frame_format in PLANAR + FULL_CHROMA:
            return (f"{self.frame_format} surface of {ws} x {hs} ({hs} luma rows at pitch {self.pitch} in a plane of {self.luma_rows}, "
                    f"then two planes of {self.chroma_rows} rows of {self.chroma_row_bytes} bytes at pitch {self.chroma_pitch}: Cb from "
                    f"byte {self.chroma_offset}, Cr from byte {self.chroma2_offset})")
        pair = "(Cr, Cb)" if self.frame_format == "nv21" else "(Cb, Cr)"
        bits = ", u16 little-endian samples" if self.frame_format == "p010" else ""
        return (f"{self.frame_format} surface of {ws} x {hs} ({hs} luma rows at pitch {self.pitch} in a plane of {self.luma_rows}, then "
                f"{hs // 2} rows of interleaved {pair} pairs at pitch {self.chroma_pitch} from byte {self.chroma_offset}{bits})")

    def __repr__(self):
        second = f", chroma2_offset={self.chroma2_offset}" if self.frame_format in PLANAR + FULL_CHROMA else ""
        return (f"SurfaceLayout({self.src_hw}, {self.frame_format!r}, pitch={self.pitch}, luma_rows={self.luma_rows}, chroma_pitch="
                f"{self.chroma_pitch}, chroma_offset={self.chroma_offset}, image_bytes={self.image_bytes}{second})")

    @classmethod
    def make(cls, layout, src_hw, frame_format):
        """None, a SurfaceLayout or a dict of its keyword arguments -> the SurfaceLayout for (src_hw, frame_format)."""
        if layout is None:
            return cls(src_hw, frame_format)
        if isinstance(layout, dict):
            return cls(src_hw, frame_format, **layout)
        if not isinstance(layout, cls):
            raise ValueError(f"layout is a SurfaceLayout or a dict of its keyword arguments, got {type(layout).__name__}")
        if layout.src_hw != (int(src_hw[0]), int(src_hw[1])) or layout.frame_format != frame_format:
            raise ValueError(f"{layout.describe()} does not describe {frame_format} frames of {int(src_hw[1])} x {int(src_hw[0])}")
        return layout


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


# ---------------------------------------------------------------------- a camera's mount roll (the reference's img.rotate)
ROLL_MAX_SIZE = 8192                                  # SIMPB_PREPROCESS_MAX_ROLL_SIZE of include/simpb_hip.h
ROLL_IDENTITY = (65536, 0, 32768, 0, 65536, 32768)    # the six integers of a level camera


def check_roll(roll):
    """A camera's roll in degrees as a float; ValueError for anything but a finite real number (a bool is not one)."""
    if isinstance(roll, (bool, np.bool_)) or not isinstance(roll, (int, float, np.integer, np.floating)) or not math.isfinite(roll):
        raise ValueError(f"a camera's roll is a finite real number of degrees, got {roll!r}")
    return float(roll)


def is_rolled(roll):
    """False where `Image.rotate(roll)` is a copy (roll % 360 == 0): that camera takes the level path."""
    return check_roll(roll) % 360.0 != 0.0


def roll_integers(roll, out_hw):
    """The six int32 (a0 .. a5) that `PIL.Image.rotate(roll)` with its defaults (nearest neighbour, no expand, about the image
    centre) comes to on an image of out_hw = (h, w): output pixel (x, y) is input pixel

        xin = (a2 + y * a1 + x * a0) >> 16,  yin = (a5 + y * a4 + x * a3) >> 16     (arithmetic shift)

    where 0 <= xin < w and 0 <= yin < h, and black elsewhere. `roll` is in degrees, positive counter-clockwise on screen.
    Restated from Pillow: Image.rotate (the matrix, rounded to 15 decimals, and the transposes it takes for 180 degrees always
    and for 90 / 270 degrees on a square image) and affine_fixed of src/libImaging/Geometry.c (FIX(v) = floor(v * 65536 + 0.5),
    the half-pixel offset folded into a2 / a5). roll % 360 == 0 gives ROLL_IDENTITY. Pillow leaves fixed point where a corner's
    source coordinate reaches 32768: a rolled image is limited to ROLL_MAX_SIZE a side, where that cannot happen (|coordinate|
    <= 3 * 8192 / 2 + 8192 * sqrt(2) < 32768)."""
    angle = check_roll(roll) % 360.0
    h, w = int(out_hw[0]), int(out_hw[1])
    if angle == 0.0:
        return ROLL_IDENTITY
    if h <= 0 or w <= 0 or h > ROLL_MAX_SIZE or w > ROLL_MAX_SIZE:
        raise ValueError(f"a rolled image is 1 .. {ROLL_MAX_SIZE} pixels a side (Pillow's fixed-point range), got {w} x {h}")
    one, half = 1 << 16, 1 << 15
    if angle == 180.0:                       # Transpose.ROTATE_180: (x, y) <- (w - 1 - x, h - 1 - y)
        return (-one, 0, (w << 16) - half, 0, -one, (h << 16) - half)
    if angle == 90.0 and w == h:             # Transpose.ROTATE_90: (x, y) <- (w - 1 - y, x)
        return (0, -one, (w << 16) - half, one, 0, half)
    if angle == 270.0 and w == h:            # Transpose.ROTATE_270: (x, y) <- (y, h - 1 - x)
        return (0, one, half, -one, 0, (h << 16) - half)
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))   # noqa: E731
    ints = (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))
    assert all(-(1 << 31) <= v < (1 << 31) for v in ints)
    return ints


def roll_matrix(roll, out_hw):
    """float64 [3, 3]: the rotation block of `_img_transform`'s matrix (augment.py:119-128) for `roll` degrees about
    (crop_w / 2, crop_h / 2), with the reference's signs; it multiplies resize, crop and flip from the left."""
    rad = check_roll(roll) / 180 * np.pi
    m = np.array([[np.cos(rad), np.sin(rad), 0], [-np.sin(rad), np.cos(rad), 0], [0, 0, 1]])
    centre = np.array([out_hw[1], out_hw[0]]) / 2
    m[:2, 2] = -m[:2, :2] @ centre + centre
    return m


def aug_matrix(aug_config, crop, flip, roll, out_hw):
    """float64 [3, 3]: what `ResizeCropFlipImage._img_transform` returns (augment.py:111-129) for a resolved crop / flip and a
    roll: resize on the diagonal, minus the crop origin, the flip, then the rotation block."""
    m = np.eye(3)
    m[:2, :2] *= (aug_config or {}).get("resize", 1)
    m[:2, 2] -= np.array(crop[:2])
    if flip:
        m = np.array([[-1, 0, crop[2] - crop[0]], [0, 1, 0], [0, 0, 1]]) @ m
    return roll_matrix(roll, out_hw) @ m if roll != 0 else m


def check_surfaces(tensors, surface):
    """A flat list of tensors, one surface (SurfaceLayout `surface`) each: u8, contiguous, all on one GPU, and each tensor's
    storage holds the image's bytes up to its last sample from data_ptr() on. Any base alignment is taken (an even one for
    p010). Returns the device."""
    import torch
    if not tensors:
        raise ValueError("ingest of an empty batch")
    need = surface.sample_end
    device = None
    for i, t in enumerate(tensors):
        if not torch.is_tensor(t) or t.dtype != torch.uint8:
            raise ValueError(f"surface {i}: ingest takes one device u8 tensor per image, each a {surface.describe()}")
        if not t.is_cuda:
            raise RuntimeError(f"surface {i} is in host memory: surfaces are read where they lie, on the GPU (there is no staging copy "
                               "and no CPU fallback in this mode)")
        device = t.device if device is None else device
        if t.device != device:
            raise ValueError(f"surface {i} is on {t.device}, surface 0 on {device}")
        if not t.is_contiguous():
            raise ValueError(f"surface {i} is a strided view {tuple(t.shape)} with strides {tuple(t.stride())}: a surface's bytes lie "
                             f"dense in memory from its first on, as a {surface.describe()}")
        have = t.untyped_storage().nbytes() - t.storage_offset()
        if have < need:
            raise ValueError(f"surface {i} holds {have} bytes from its first: a {surface.describe()} has its last sample at byte {need}")
        if surface.frame_format == "p010" and t.data_ptr() % 2:
            raise ValueError(f"surface {i} starts at an odd address: p010 samples are 16-bit words")
    return device


def _rolls(roll):
    """`roll` of a ResamplePlan as a tuple of floats: a number (one roll for every image), or a sequence of 1 .. 16 of them
    (image n takes entry n % len: one per camera of a runner's [bs, cams] batch)."""
    if isinstance(roll, (list, tuple, np.ndarray)):
        rolls = tuple(check_roll(r) for r in roll)
        if not 1 <= len(rolls) <= RIG_MAX_CAMS:
            raise ValueError(f"a list of rolls has 1 .. {RIG_MAX_CAMS} entries (one per camera), got {len(rolls)}")
        return rolls
    return (check_roll(roll),)


def plan_key(src_hw, aug_config, frame_format="bgr", colour="jfif", layout=None, roll=0.0, chroma="replicate"):
    """What a ResamplePlan depends on: a frame whose key differs must not run on the plan's tables (nor a frame of another
    format or colour standard on the plan's kernel; the standard says nothing about BGR, RGB, BGRA or RGBA frames and is left
    out of their key).
    `layout` (a SurfaceLayout or a dict of its keyword arguments) adds its own key unless it is tight: a frame never runs on a
    plan, or a captured graph, made for another layout.
    `roll` (degrees; a number or one per camera) adds its own entry where a camera is rolled (roll % 360 != 0), and nothing
    otherwise: every key of a level plan is what it was, and a frame never runs on the integers of another roll.
    `chroma` ("replicate" | "jpeg") adds ("chroma", "jpeg") where chroma is interpolated, and nothing otherwise."""
    _check_format(frame_format, colour, chroma)
    dims, crop, flip = resolve_aug(src_hw, aug_config)
    key = (int(src_hw[0]), int(src_hw[1]), dims, crop, flip, frame_format, colour if frame_format not in RGB_ORDER else None)
    extra = None if layout is None else SurfaceLayout.make(layout, src_hw, frame_format).key
    key = key if extra is None else key + (extra,)
    rolls = _rolls(roll)
    key = key + (("roll",) + tuple(r % 360.0 for r in rolls),) if any(is_rolled(r) for r in rolls) else key
    return key + (("chroma", chroma),) if chroma != "replicate" else key


def _device(device):
    """torch.device with its index spelled out ("cuda" and "cuda:0" name the same tables)."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class _Resident:
    """The device side that a ResamplePlan and a RigPlan have alike: `_dev`, a dict of what is resident on one device (the tables
    the plan's `upload` names, `pitch`, the intermediate buffer `mid` and the address table `table`, both made on first use and
    kept), the output's rule, and the address table behind `run_surfaces` / `run_table`."""

    _dev = None

    def _upload(self, device, plans, **arrays):
        """`arrays` (numpy) onto `device` as the new `_dev`; ValueError where a plan of `plans` is outside the kernel's limits."""
        import torch
        from . import _lib
        for p in plans:
            if p.taps_x > 64 or p.taps_y > 64 or p.src_hw[1] > 4096 or p.out_hw[1] > 2048:
                raise ValueError(f"ingest of {p.src_hw} -> {p.resize_dims} is outside the kernel's limits "
                                 "(source width 4096, output width 2048, 64 taps)")
        device = _device(device)
        self._dev = dict(device=device, pitch=int(_lib.lib().simpb_preprocess_mid_pitch(self.out_hw[1])), mid=None, table=None,
                         **{name: torch.from_numpy(np.ascontiguousarray(a)).to(device) for name, a in arrays.items()})
        return self

    def _resident(self, device):
        """`_dev` on `device` (uploaded now unless it is there already)."""
        if self._dev is None or self._dev["device"] != _device(device):
            self.upload(device)
        return self._dev

    def _reserve_mid(self, device, rows):
        """The intermediate buffer of at least `rows` rows (of all images together) on `device`."""
        d = self._resident(device)
        if d["mid"] is None or d["mid"].numel() < rows * d["pitch"]:
            import torch
            d["mid"] = torch.empty(rows * d["pitch"], dtype=torch.uint8, device=d["device"])
        return self

    def intermediate(self):
        """The u8 intermediate buffer of the last launch (None before the first `reserve`): what tools/ingest_bits.py compares."""
        return None if self._dev is None else self._dev["mid"]

    def _out(self, out, n, device):
        """The output of `n` images: `out` checked, or a new tensor."""
        import torch
        h, w = self.out_hw
        if out is None:
            return torch.empty(n, h, w, 4, dtype=torch.float16, device=device)
        if out.dtype != torch.float16 or tuple(out.shape) != (n, h, w, 4) or not out.is_contiguous():
            raise ValueError(f"ingest writes f16 [{n}, {h}, {w}, 4]")
        return out

    def run_surfaces(self, tensors, out=None):
        """One device u8 tensor per image (a flat list; each its own allocation, or a view into one) -> f16 [N, h, w, 4] as
        `run`. The addresses go into a resident int64 table that the launch reads; the tensors must stay alive and unchanged
        until the launch has run. (A rig: streams * cams of them, None where an image is skipped.)"""
        import torch
        ptrs, device = self.surface_table(tensors)
        n = len(ptrs)
        self.reserve(n, device)
        d = self._dev
        if d["table"] is None or d["table"].numel() < n:
            d["table"] = torch.zeros(n, dtype=torch.int64, device=d["device"])
        # (a copy out of pageable memory: the host buffer is free again when the call returns)
        d["table"][:n].copy_(torch.tensor(ptrs, dtype=torch.int64))
        return self.run_table(d["table"][:n], out)

    @staticmethod
    def _check_table(table):
        """The number of addresses of a `run_table` argument; ValueError unless it is a contiguous device int64 tensor."""
        import torch
        if table.dtype != torch.int64 or not table.is_cuda or not table.is_contiguous() or table.numel() == 0:
            raise ValueError("the surface table is a contiguous device int64 tensor with one address per image")
        return int(table.numel())


class ResamplePlan(_Resident):
    """Tables of one ingest configuration; `upload(device)` makes them resident, `run(frames)` launches.

    frame_format "bgr": u8 [..., Hs, Ws, 3] interleaved pixels. "nv12" / "nv21": one image is a contiguous u8 [Hs * 3 / 2, Ws]:
    rows 0 .. Hs - 1 are luma, rows Hs .. Hs * 3 / 2 - 1 interleaved chroma pairs, (Cb, Cr) for nv12 and (Cr, Cb) for nv21;
    chroma sample (i, j) belongs to luma rows 2i, 2i + 1 and columns 2j, 2j + 1 and is replicated, not interpolated (the
    antialiased bicubic reduction behind it makes the choice of chroma up-sampler immaterial). Hs and Ws are even and the row
    pitch is Ws (a decoder's padded pitch needs `layout`). `colour` names the standard of `yuv_coefficients`. The converted
    pixel is staged as (B, G, R), so to_rgb, the table and the output mean what they mean for BGR frames: the output equals
    the BGR plan's on the converted frames bit for bit.

    "p010": the same arrangement in u16 little-endian samples (sample = word >> 6; `p010_coefficients`), given as bytes: u8
    [Hs * 3 / 2, Ws * 2]. `layout` (a SurfaceLayout or a dict of its keyword arguments) describes a decoder's padded surface
    instead: one image is then u8 [image_bytes], `run` takes a contiguous batch of them and `run_surfaces` one tensor per
    image. Without a layout (or with a tight one) the plan is the one described above.

    "yuv420p" / "yvu420p" (I420 / YV12, a software decoder's planar 4:2:0): u8 [Hs * 3 / 2, Ws], Hs luma rows, then the Cb
    plane and the Cr plane (yvu420p: Cr, then Cb) of Hs / 2 rows of Ws / 2 bytes each; chroma replicated as for nv12. "yuyv" /
    "uyvy" (packed 4:2:2): u8 [Hs, Ws, 2], groups of (Y0, Cb, Y1, Cr) / (Cb, Y0, Cr, Y1), the pair belongs to columns 2j, 2j + 1
    of its own row; Ws even, any Hs. "rgb": u8 [Hs, Ws, 3], R first. "bgra" / "rgba": u8 [Hs, Ws, 4], byte 3 ignored. The
    YCbCr forms follow `colour` like nv12; the others are a byte permutation into the staged (B, G, R) row and `colour` is not
    looked at. All take `layout` (SurfaceLayout has their fields) and `run_surfaces`.

    `roll`: the camera's mount roll in degrees, positive counter-clockwise on screen -- the reference's fourth step,
    `img.rotate(rotate)` (augment.py:92,105), behind resize, crop and flip, with Pillow's bytes (`roll_integers`); black
    corners are normalised like any pixel. A number, or one per camera (image n takes roll[n % len]). It is a property of the
    mount and is given beside the aug_config, whose own `rotate` stays refused (0 in the reference's test mode). A plan
    without a rolled camera launches exactly what it launched before. The 2D records do not change: the reference's
    decode_box2d (detection3d/decoder.py:36-51) does not look at rotate.

    "yuv444p": u8 [Hs * 3, Ws], the luma, Cb and Cr planes of Hs rows of Ws bytes, any size: what a 4:4:4 JPEG decodes to.
    `chroma="jpeg"` (nv12, nv21, yuv420p, yvu420p, yuyv, uyvy): the chroma samples are centre-sited and every pixel gets its own
    Cb / Cr by libjpeg's "fancy" upsampling, the triangle filter its decoder applies to a JPEG at its defaults, in integers
    (include/simpb_hip.h has the rule). With colour="jpeg" -- libjpeg's own four constants -- the native planes of a JPEG give
    the bytes libjpeg decodes from that file: what the reference's loader (mmcv.imread) would have handed on from the same
    coefficients. Pinned to libjpeg-turbo through Pillow for 4:2:0, 4:4:4 and the constants (tests/test_chroma_host.py); the
    4:2:2 rule is stated from libjpeg's published algorithm, which hands out no native 4:2:2 planes to pin it to. In every
    layout and with `roll`; a tight nv12 / nv21 batch then takes the surface kernel. "replicate" (default): nothing changes."""

    def __init__(self, src_hw, aug_config=None, img_norm_cfg=None, frame_format="bgr", colour="jfif", layout=None, roll=0.0,
                 chroma="replicate"):
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        _check_format(frame_format, colour, chroma)
        self.frame_format, self.colour, self.chroma = frame_format, colour, chroma
        self.surface = SurfaceLayout.make(layout, self.src_hw, frame_format)
        self.frame_shape = frame_shape(self.src_hw, frame_format) if self.surface.tight else (self.surface.image_bytes,)
        self.yuv = None if frame_format in RGB_ORDER else yuv_coefficients(colour)
        self.resize_dims, self.crop, self.flip = resolve_aug(self.src_hw, aug_config)
        self.rolls = _rolls(roll)
        self.rolled = any(is_rolled(r) for r in self.rolls)
        self.aug_config = dict(aug_config or {})
        self.key = plan_key(self.src_hw, aug_config, frame_format, colour, self.surface, roll, chroma)
        cfg = IMG_NORM_CFG if img_norm_cfg is None else img_norm_cfg
        self.img_norm_cfg = dict(mean=list(cfg["mean"]), std=list(cfg["std"]), to_rgb=bool(cfg.get("to_rgb", True)))
        self.swap_rb = self.img_norm_cfg["to_rgb"]
        x0, y0, x1, y1 = self.crop
        self.out_hw = (y1 - y0, x1 - x0)
        # int32 [cams][6], identity rows for the level cameras (None: no camera is rolled)
        self.roll_ints = np.asarray([roll_integers(r, self.out_hw) for r in self.rolls], np.int32) if self.rolled else None
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

    def image_transform(self, camera=0):
        """float64 [3, 3]: the matrix `ResizeCropFlipImage._img_transform` returns (augment.py:111-129) for this plan and the
        roll of `camera` (its entry of a list of rolls): resize, minus the crop origin, the flip, then the rotation block about
        (crop_w / 2, crop_h / 2). A caller multiplies it into the camera's intrinsics, as the reference's pipeline does."""
        return aug_matrix(self.aug_config, self.crop, self.flip, self.rolls[camera % len(self.rolls)], self.out_hw)

    # ------------------------------------------------------------------ traffic the algorithm needs (tools/bench_preprocess.py)
    def bytes_per_image(self, mid_pitch):
        h, w = self.out_hw
        mid = self.src_rows * mid_pitch
        if self.frame_format in PIXEL_BYTES:   # one plane: a 4:2:2 row carries its own chroma, and the alpha bytes count as read
            source = self.src_rows * self.surface.row_bytes
        else:   # the needed luma rows and the distinct chroma rows under them (needed bytes: both luma rows of a pair stage it)
            last = self.src_row0 + self.src_rows - 1
            if self.frame_format in FULL_CHROMA:
                chroma_rows = self.src_rows
            elif self.chroma == "jpeg":   # the far rows as well: one above an even first row and one below an odd last row
                hc = self.src_hw[0] // 2
                lo = max((self.src_row0 >> 1) - (0 if self.src_row0 & 1 else 1), 0)
                chroma_rows = min((last >> 1) + (1 if last & 1 else 0), hc - 1) - lo + 1
            else:
                chroma_rows = (last >> 1) - (self.src_row0 >> 1) + 1
            planes = 2 if self.frame_format in PLANAR + FULL_CHROMA else 1
            source = self.src_rows * self.surface.row_bytes + chroma_rows * planes * self.surface.chroma_row_bytes   # (no padding)
        return dict(source=source, mid_write=mid, mid_read=mid, out=h * w * 8)

    # ------------------------------------------------------------------ device
    def upload(self, device):
        return self._upload(device, (self,), kx=self.kx, xlo=self.xlo, xn=self.xn, ky=self.ky, ylo=self.ylo, yn=self.yn, lut=self.lut)

    def reserve(self, num_images, device):
        """Allocate the intermediate buffer for `num_images` now (a runner does this before any graph capture)."""
        return self._reserve_mid(device, num_images * self.src_rows)

    def layout(self):
        """The frames `run` takes, in words (for error messages)."""
        hs, ws = self.src_hw
        if not self.surface.tight:
            return f"u8 [..., {self.surface.image_bytes}] images, each a {self.surface.describe()}"
        if self.frame_format == "bgr":
            return f"u8 [..., {hs}, {ws}, 3] frames (interleaved BGR)"
        if self.frame_format in PIXEL_BYTES:
            return (f"u8 [..., {hs}, {ws}, {PIXEL_BYTES[self.frame_format]}] {self.frame_format} frames "
                    f"({SurfaceLayout.PIXELS[self.frame_format]}; a padded surface needs layout=)")
        if self.frame_format in PLANAR:
            order = "Cb plane, then the Cr plane" if self.frame_format == "yuv420p" else "Cr plane, then the Cb plane"
            return (f"u8 [..., {hs * 3 // 2}, {ws}] {self.frame_format} frames ({hs} luma rows of {ws} bytes, then the {order}, each "
                    f"{hs // 2} rows of {ws // 2} bytes; a padded surface needs layout=)")
        if self.frame_format in FULL_CHROMA:
            return (f"u8 [..., {hs * 3}, {ws}] {self.frame_format} frames (the luma, Cb and Cr planes, {hs} rows of {ws} bytes each; a "
                    f"padded surface needs layout=)")
        if self.frame_format == "p010":
            return (f"u8 [..., {hs * 3 // 2}, {ws * 2}] p010 frames (the bytes of u16 little-endian samples: {hs} luma rows, then {hs // 2} "
                    f"rows of interleaved (Cb, Cr) pairs, row pitch {ws * 2}; a padded surface needs layout=)")
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
        """frames u8 [..., Hs, Ws, 3] (u8 [..., Hs * 3 / 2, Ws] for nv12 / nv21, [..., Hs * 3 / 2, Ws * 2] for p010, [..., image_bytes]
        with a padded layout) on the device (contiguous) -> f16 [N, h, w, 4] (N = product of the leading dimensions), channel
        3 = 0. Launches on the current stream; the intermediate buffer is allocated on first use and kept."""
        self.check_frames(frames)
        if not frames.is_cuda:
            raise RuntimeError("simpb_amd operators run on the GPU only (got a CPU tensor); there is no CPU fallback")
        if not frames.is_contiguous():
            raise ValueError("ingest takes contiguous frames" + (" (interleaved pixels)" if self.frame_format in RGB_ORDER else ""))
        n = int(frames.numel() // int(np.prod(self.frame_shape)))
        if n == 0:
            raise ValueError("ingest of an empty batch")
        if self.frame_format == "p010" and frames.data_ptr() % 2:
            raise ValueError("p010 frames are 16-bit words: the batch starts at an odd address")
        return self._launch(n, frames.device, out, src=frames)

    def surface_table(self, tensors):
        """(addresses, device) of a flat list of device u8 tensors, one surface each, checked by `check_surfaces`."""
        tensors = list(tensors)
        return [t.data_ptr() for t in tensors], check_surfaces(tensors, self.surface)

    def run_table(self, table, out=None):
        """table: device int64 [...], contiguous: the address of one surface per image (as `surface_table` checks them). The
        launch reads the table when it runs, so a captured launch follows the addresses written into it before each replay."""
        return self._launch(self._check_table(table), table.device, out, table=table)

    def _launch(self, n, device, out, src=None, table=None):
        import torch
        from . import _lib
        self.reserve(n, device)
        d, sf, code = self._dev, self.surface, format_code(self.frame_format, self.chroma)
        out = self._out(out, n, device)
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        tables = (p(d["mid"]), p(d["kx"]), p(d["xlo"]), p(d["xn"]), p(d["ky"]), p(d["ylo"]), p(d["yn"]), p(d["lut"]))
        ints = (n, *self.src_hw, *self.out_hw, self.taps_x, self.taps_y, self.src_row0, self.src_rows, int(self.flip), int(self.swap_rb))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def images():   # both forms of the images, exactly one of them given
            null = ctypes.c_void_p(0)
            return (p(src), null) if table is None else (null, p(table))

        def layout(*second):   # what a surface entry point takes behind the ints (`second`: chroma2_offset, where it has one)
            yuv = self.yuv if self.yuv is not None else (0, 1, 0, 0, 0, 0)
            return (code, sf.pitch, sf.chroma_pitch, sf.chroma_offset, *second, sf.image_bytes, *yuv)

        # the one decision: which entry point, and what it takes in front of the tables and between the ints and the stream
        tight = table is None and sf.tight
        if self.rolled:   # one entry point for every format and layout (the planes entry point's arguments, then the roll)
            rows = self.roll_ints.ctypes.data_as(ctypes.POINTER(ctypes.c_int))   # (read before the call returns)
            name, head, tail = "simpb_preprocess_roll_nhwc4_f16", images(), (*layout(sf.chroma2_offset), rows, len(self.rolls))
        elif tight and self.frame_format == "bgr":   # the first forms, through their entry points
            name, head, tail = "simpb_preprocess_u8_nhwc4_f16", (p(src),), ()
        elif tight and self.frame_format in ("nv12", "nv21") and self.chroma == "replicate":
            name, head, tail = "simpb_preprocess_yuv420sp_nhwc4_f16", (p(src),), (int(self.frame_format == "nv21"), *self.yuv)
        elif code <= SURFACE_FORMAT["p010"]:
            name, head, tail = "simpb_preprocess_surface_nhwc4_f16", images(), layout()
        else:   # planar 4:2:0 and 4:4:4, packed 4:2:2, the RGB-order family, and every format with interpolated chroma
            name, head, tail = "simpb_preprocess_planes_nhwc4_f16", images(), layout(sf.chroma2_offset)
        _lib.check(getattr(_lib.lib(), name)(p(out), *head, *tables, *ints, *tail, stream), name)
        return out


# ---------------------------------------------------------------------- a rig of cameras that differ
RIG_MAX_CAMS = 16     # SIMPB_RIG_MAX_CAMS of include/simpb_hip.h


class CameraSource:
    """One camera of a rig (RigPlan): what a ResamplePlan takes for that camera alone, with the same checks. A camera of a
    rig gives its scale as the reference's scalar `resize` (with `crop` and `flip`): the 2D boxes are mapped back to source
    pixels by that scalar (decoder.py:36-51), so an explicit, possibly anisotropic `resize_dims` is refused. `roll`: this
    camera's mount roll in degrees; `chroma`: "replicate" | "jpeg", this camera's chroma (ResamplePlan has both rules)."""

    def __init__(self, src_hw, aug_config=None, frame_format="bgr", colour="jfif", layout=None, roll=0.0, chroma="replicate"):
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.roll = check_roll(roll)
        self.aug_config = dict(aug_config or {})
        if self.aug_config.get("resize_dims") is not None:
            raise ValueError("a camera of a rig gives its scale as `resize` (with crop / flip): resize_dims is not taken, the 2D "
                             "boxes are mapped back to source pixels by the reference's isotropic rule")
        _check_format(frame_format, colour, chroma)
        self.frame_format, self.colour, self.chroma = frame_format, colour, chroma
        self.surface = SurfaceLayout.make(layout, self.src_hw, frame_format)
        self.resize = float(self.aug_config.get("resize", 1))
        self.resize_dims, self.crop, self.flip = resolve_aug(self.src_hw, self.aug_config)
        self.out_hw = (self.crop[3] - self.crop[1], self.crop[2] - self.crop[0])
        self.key = plan_key(self.src_hw, self.aug_config, frame_format, colour, self.surface, self.roll, chroma) + (self.resize,)

    def plan(self, img_norm_cfg=None):
        """The ResamplePlan of this camera alone."""
        return ResamplePlan(self.src_hw, self.aug_config, img_norm_cfg, self.frame_format, self.colour, self.surface, self.roll,
                            self.chroma)

    def describe(self):
        return f"{self.frame_format}{' (jpeg chroma)' if self.chroma == 'jpeg' else ''} {self.src_hw[1]} x {self.src_hw[0]} -> {self.out_hw[1]} x {self.out_hw[0]}"


class RigPlan(_Resident):
    """Tables of a rig of 1 .. 16 cameras that may differ in source size, format, colour standard, surface layout, resize, crop
    and flip, and give one output size: per camera exactly what its own ResamplePlan holds (`plans`), concatenated camera
    by camera for the device, and one normalisation table. A rig takes surfaces only -- one device u8 tensor per image, in
    (stream, camera) order -- since images of different sizes have no common tensor; None in place of a tensor (address 0 in
    the table) skips that image: nothing is read for it and its output block is zeros."""

    TABLES = ("kx", "xlo", "xn", "ky", "ylo", "yn")

    def __init__(self, sources, img_norm_cfg=None):
        sources = list(sources)
        if not 1 <= len(sources) <= RIG_MAX_CAMS:
            raise ValueError(f"a rig has 1 .. {RIG_MAX_CAMS} cameras, got {len(sources)}")
        for i, s in enumerate(sources):
            if not isinstance(s, CameraSource):
                raise ValueError(f"camera {i} of the rig is a {type(s).__name__}: a rig is a list of preprocess.CameraSource")
        if len({s.out_hw for s in sources}) != 1:
            sizes = ", ".join(f"camera {i}: {s.out_hw[1]} x {s.out_hw[0]}" for i, s in enumerate(sources))
            raise ValueError(f"the cameras of a rig give one output size (the backbone takes one), got {sizes}")
        self.sources = tuple(sources)
        self.num_cams = len(sources)
        self.plans = tuple(s.plan(img_norm_cfg) for s in sources)
        p0 = self.plans[0]
        self.out_hw, self.img_norm_cfg, self.swap_rb, self.lut = p0.out_hw, p0.img_norm_cfg, p0.swap_rb, p0.lut
        self.key = ("rig",) + tuple(s.key for s in sources)
        # per camera: the plan's own arrays and numbers
        for name in self.TABLES:
            setattr(self, name, tuple(getattr(p, name) for p in self.plans))
        for name in ("taps_x", "taps_y", "src_row0", "src_rows", "flip"):
            setattr(self, name, tuple(getattr(p, name) for p in self.plans))
        self.yuv = tuple(p.yuv for p in self.plans)
        self.surfaces = tuple(p.surface for p in self.plans)
        # a rig with a rolled camera: int32 [cams][6], identity rows for its level cameras (None: today's entry point)
        self.rolled = any(p.rolled for p in self.plans)
        self.roll_ints = np.asarray([roll_integers(s.roll, self.out_hw) for s in sources], np.int32) if self.rolled else None
        # where each camera's tables start in the concatenation, and its rows in one stream's intermediate block
        ends = lambda sizes: [int(v) for v in np.concatenate([[0], np.cumsum(sizes)])]   # noqa: E731
        self.kx_offset, self.x_offset = ends([k.size for k in self.kx]), ends([v.size for v in self.xlo])
        self.ky_offset, self.y_offset = ends([k.size for k in self.ky]), ends([v.size for v in self.ylo])
        self.mid_row = ends(self.src_rows)
        self.mid_rows = self.mid_row[-1]

    # ------------------------------------------------------------------ what a caller multiplies / hands on
    def image_transforms(self):
        """float64 [cams, 3, 3]: per camera the matrix `ResizeCropFlipImage._img_transform` returns (augment.py:111-129):
        resize on the diagonal, minus the crop origin, the flip, then the rotation block of the camera's roll about
        (crop_w / 2, crop_h / 2) (nothing for a level camera). A caller multiplies it into the camera's intrinsics, as the
        reference's pipeline does."""
        out = np.zeros((self.num_cams, 3, 3), np.float64)
        for i, s in enumerate(self.sources):
            out[i] = aug_matrix(s.aug_config, s.crop, s.flip, s.roll, s.out_hw)
        return out

    def box2d_table(self):
        """float32 [cams, 4] = (crop_w, crop_h, crop_y0, 1 / resize) per camera: what the 2D record kernels take as four
        scalars for a uniform rig (1 / resize in fp32, as simpb_decode2d_record computes it). A camera's roll does not enter:
        the reference's decode_box2d (detection3d/decoder.py:36-51) does not look at rotate."""
        out = np.zeros((self.num_cams, 4), np.float32)
        for i, s in enumerate(self.sources):
            x0, y0, x1, y1 = s.crop
            out[i] = (x1 - x0, y1 - y0, y0, np.float32(1.0) / np.float32(s.resize))
        return out

    def box2d_device(self, device):
        """`box2d_table` on the device (resident: a captured 2D record reads it)."""
        return self._resident(device)["box2d"]

    def descriptors(self):
        """The rig as the host array of simpb_rig_camera that simpb_preprocess_rig_nhwc4_f16 takes."""
        from . import _lib
        cams = (_lib.RigCamera * self.num_cams)()
        for i, (p, c) in enumerate(zip(self.plans, cams)):
            sf = p.surface
            c.format, c.src_height, c.src_width = format_code(p.frame_format, p.chroma), p.src_hw[0], p.src_hw[1]
            c.src_row0, c.src_rows, c.taps_x, c.taps_y, c.flip = p.src_row0, p.src_rows, p.taps_x, p.taps_y, int(p.flip)
            c.pitch, c.chroma_pitch, c.chroma_offset, c.chroma2_offset = sf.pitch, sf.chroma_pitch, sf.chroma_offset, sf.chroma2_offset
            c.kx_offset, c.x_offset, c.ky_offset, c.y_offset = self.kx_offset[i], self.x_offset[i], self.ky_offset[i], self.y_offset[i]
            c.mid_row = self.mid_row[i]
            c.yoff, c.iy, c.irv, c.igu, c.igv, c.ibu = p.yuv if p.yuv is not None else (0, 1, 0, 0, 0, 0)
        return cams

    # ------------------------------------------------------------------ device
    def upload(self, device):
        cat = lambda name: np.concatenate([a.reshape(-1) for a in getattr(self, name)])   # noqa: E731
        self._upload(device, self.plans, lut=self.lut, box2d=self.box2d_table(), **{n: cat(n) for n in self.TABLES})
        self._dev["cams"] = self.descriptors()
        return self

    def reserve(self, num_images, device):
        """Allocate the intermediate buffer for `num_images` (whole streams) now (a runner does this before any capture)."""
        if num_images <= 0 or num_images % self.num_cams:
            raise ValueError(f"a rig of {self.num_cams} cameras takes whole streams: {num_images} images")
        return self._reserve_mid(device, num_images // self.num_cams * self.mid_rows)

    def surface_table(self, tensors):
        """(addresses, device) of a flat list of streams * cams device u8 tensors in (stream, camera) order, each checked by
        `check_surfaces` against its own camera's layout; None gives address 0 (the image is skipped)."""
        tensors = list(tensors)
        if not tensors or len(tensors) % self.num_cams:
            raise ValueError(f"a rig of {self.num_cams} cameras takes whole streams of surfaces, got {len(tensors)}")
        device = None
        for c, p in enumerate(self.plans):
            mine = [t for t in tensors[c::self.num_cams] if t is not None]
            if not mine:
                continue
            try:
                dev = check_surfaces(mine, p.surface)
            except (ValueError, RuntimeError) as e:
                raise type(e)(f"camera {c} of the rig: {e}") from None
            device = dev if device is None else device
            if dev != device:
                raise ValueError(f"camera {c} of the rig: its surfaces are on {dev}, the others on {device}")
        if device is None:
            raise ValueError("ingest of a rig without a single surface")
        return [0 if t is None else t.data_ptr() for t in tensors], device

    def run_table(self, table, out=None):
        """table: device int64 [...], contiguous, streams * cams addresses (as `surface_table` checks them; 0 skips the image).
        The launch reads the table when it runs, so a captured launch follows the addresses written before each replay."""
        import torch
        from . import _lib
        n, (h, w) = self._check_table(table), self.out_hw
        self.reserve(n, table.device)
        d = self._dev
        out = self._out(out, n, table.device)
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        args = (p(out), p(table), p(d["mid"]), *(p(d[name]) for name in self.TABLES), p(d["lut"]), d["cams"], self.num_cams, n, h, w,
                d["kx"].numel(), d["xlo"].numel(), d["ky"].numel(), d["ylo"].numel(), self.mid_rows, int(self.swap_rb))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.rolled:
            rows = self.roll_ints.ctypes.data_as(ctypes.POINTER(ctypes.c_int))   # (read before the call returns)
            _lib.check(_lib.lib().simpb_preprocess_rig_roll_nhwc4_f16(*args, rows, stream), "simpb_preprocess_rig_roll_nhwc4_f16")
        else:
            _lib.check(_lib.lib().simpb_preprocess_rig_nhwc4_f16(*args, stream), "simpb_preprocess_rig_nhwc4_f16")
        return out
