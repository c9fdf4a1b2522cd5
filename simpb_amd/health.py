"""Camera health: which cameras of a frame delivered a usable image, decided on the device right behind the ingest
(csrc/health.hip; include/simpb_hip.h, "Camera health"). `CameraHealth` is the configuration a runner takes as
`camera_health=`; `image_health_stats` and `camera_health_verdict` are thin wrappers of the two launches. There is no CPU or
PyTorch form of either: tests/health_ref.py is the numpy model they are checked against, bit for bit."""
import ctypes
import math
import numbers

import numpy as np

GRID = 8            # SIMPB_HEALTH_GRID
BANDS = 64          # SIMPB_HEALTH_BANDS
PARTIAL_WORDS = 26  # SIMPB_HEALTH_PARTIAL_WORDS
DARK, BRIGHT, FLAT, FROZEN, FAIL_OPEN, NONFINITE = 1, 2, 4, 8, 16, 32
FAULTS = DARK | BRIGHT | FLAT | FROZEN | NONFINITE
FLAG_NAMES = {DARK: "dark", BRIGHT: "bright", FLAT: "flat", FROZEN: "frozen", FAIL_OPEN: "fail_open", NONFINITE: "nonfinite"}


def describe(flags):
    """The names of the bits set in one flags byte, e.g. describe(9) == ("dark", "frozen")."""
    return tuple(name for bit, name in FLAG_NAMES.items() if int(flags) & bit)


class CameraHealth:
    """What `camera_health=` of the runners takes. Levels are 0..255 of the preprocessed image (the normalisation undone).
    dark_below / bright_above: a camera whose mean level is below / above is dark / bright; flat_below: one whose 8 x 8 cell
    levels spread less than this is flat (a covered or fogged lens); frozen_after: one that delivered the same pixels again
    this many times in a row is frozen (1: the first repeat). None switches a check off. act=False: the flags are reported,
    no camera is dropped."""

    def __init__(self, dark_below=16.0, bright_above=240.0, flat_below=2.0, frozen_after=2, act=True):
        for name, v in (("dark_below", dark_below), ("bright_above", bright_above), ("flat_below", flat_below)):
            if v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
                raise ValueError(f"camera_health: {name}={v!r} is a finite number or None")
        if flat_below is not None and flat_below < 0:
            raise ValueError(f"camera_health: flat_below={flat_below!r} is a spread of levels: not negative")
        if dark_below is not None and bright_above is not None and not dark_below < bright_above:
            raise ValueError(f"camera_health: dark_below={dark_below!r} is not below bright_above={bright_above!r}: every image "
                             "would be one or the other")
        if frozen_after is not None:
            if isinstance(frozen_after, bool) or not isinstance(frozen_after, numbers.Integral) or frozen_after < 1:
                raise ValueError(f"camera_health: frozen_after={frozen_after!r} is an int >= 1 (the number of repeats) or None")
        if not isinstance(act, (bool, np.bool_)):
            raise ValueError(f"camera_health: act={act!r} is a bool")
        self.dark_below = None if dark_below is None else float(dark_below)
        self.bright_above = None if bright_above is None else float(bright_above)
        self.flat_below = None if flat_below is None else float(flat_below)
        self.frozen_after = None if frozen_after is None else int(frozen_after)
        self.act = bool(act)

    @classmethod
    def make(cls, value):
        """A CameraHealth as it is, a dict of the constructor's keywords, or True for the defaults."""
        if isinstance(value, cls):
            return value
        if value is True:
            return cls()
        if isinstance(value, dict):
            return cls(**value)
        raise ValueError(f"camera_health is a CameraHealth, a dict of its keywords or True, not {type(value).__name__}")

    def __repr__(self):
        return (f"CameraHealth(dark_below={self.dark_below}, bright_above={self.bright_above}, flat_below={self.flat_below}, "
                f"frozen_after={self.frozen_after}, act={self.act})")

    def params(self, img_norm_cfg=None):
        """simpb_health_params for the launch: the thresholds with mean / std of the normalisation, in the channel order of
        the normalised tensor (img_norm_cfg as the ingest takes it; None: the shipped configs')."""
        from . import _lib
        from .preprocess import IMG_NORM_CFG
        cfg = IMG_NORM_CFG if img_norm_cfg is None else img_norm_cfg
        mean, std = [float(v) for v in cfg["mean"]], [float(v) for v in cfg["std"]]
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("img_norm_cfg: three means and three stds")
        on = lambda v: 0.0 if v is None else v   # noqa: E731
        return _lib.HealthParams(on(self.dark_below), on(self.bright_above), on(self.flat_below), (ctypes.c_double * 3)(*mean),
                                 (ctypes.c_double * 3)(*std), int(self.dark_below is not None), int(self.bright_above is not None),
                                 int(self.flat_below is not None), int(self.frozen_after is not None), self.frozen_after or 0,
                                 int(self.act))


def partials_bytes(num_images, height, width):
    """Bytes of the partial rows `image_health_stats` writes for num_images images of height x width."""
    from . import _lib
    n = _lib.lib().simpb_image_health_partials_bytes(int(num_images), int(height), int(width))
    if n == 1:
        raise ValueError(f"camera health takes 1..65535 images of 8..16384 rows and columns, not {num_images} of {height} x {width}")
    return n


def new_state(batch_size, num_cams, device):
    """The persistent state of the frozen check, all zero: int64 [batch_size, num_cams, 2] (simpb_health_state: prev_hash,
    then repeats in the low and frames in the high half of the second word)."""
    import torch
    return torch.zeros(batch_size, num_cams, 2, dtype=torch.int64, device=device)


def state_to_host(state):
    """A state tensor -> dict(prev_hash u64, repeats u32, frames u32), each [batch_size, num_cams] numpy (a copy)."""
    words = state.detach().cpu().numpy().view(np.uint64)
    return dict(prev_hash=words[..., 0].copy(), repeats=(words[..., 1] & np.uint64(0xFFFFFFFF)).astype(np.uint32),
                frames=(words[..., 1] >> np.uint64(32)).astype(np.uint32))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def image_health_stats(images, out=None):
    """images f16 [N, H, W, 4] on the device (the ingest's output, contiguous; a view that starts 8 bytes into a 16-byte
    line is taken) -> the partial rows, int64 [N, 64, 26]. One launch on the current stream."""
    import torch
    from . import _lib
    if not torch.is_tensor(images) or images.dtype != torch.float16 or images.dim() != 4 or images.shape[3] != 4:
        raise ValueError("image_health_stats takes f16 [N, H, W, 4]")
    if not images.is_cuda:
        raise RuntimeError("simpb_amd operators run on the GPU only (got a CPU tensor); there is no CPU fallback")
    if not images.is_contiguous():
        raise ValueError("image_health_stats takes contiguous images")
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    size = partials_bytes(n, h, w)
    if out is None:
        out = torch.empty(n, BANDS, PARTIAL_WORDS, dtype=torch.int64, device=images.device)
    elif out.dtype != torch.int64 or out.numel() * 8 != size or not out.is_contiguous() or out.device != images.device:
        raise ValueError(f"image_health_stats writes int64 [{n}, {BANDS}, {PARTIAL_WORDS}] on the images' device")
    _lib.check(_lib.lib().simpb_image_health_stats(_ptr(out), _ptr(images), n, h, w, _stream()), "simpb_image_health_stats")
    return out


def camera_health_verdict(partials, state, params, image_hw, cam_in=None, active=None, cam_out=None, flags=None):
    """One verdict launch on the current stream. partials int64 [bs * cams, 64, 26]; state int64 [bs, cams, 2] (new_state),
    read and written; params: CameraHealth.params(...); cam_in u8 [bs, cams] / active u8 [bs] or None (all ones).
    Returns (cam_out, flags), u8 [bs, cams] each (written into the given tensors where given)."""
    import torch
    from . import _lib
    if state.dtype != torch.int64 or state.dim() != 3 or state.shape[2] != 2 or not state.is_contiguous() or not state.is_cuda:
        raise ValueError("the health state is a contiguous device int64 [bs, cams, 2] (health.new_state)")
    bs, cams = int(state.shape[0]), int(state.shape[1])
    dev = state.device
    if (partials.dtype != torch.int64 or not partials.is_contiguous() or partials.device != dev
            or partials.numel() != bs * cams * BANDS * PARTIAL_WORDS):
        raise ValueError(f"the partial rows of {bs} x {cams} images are a contiguous int64 [{bs * cams}, {BANDS}, {PARTIAL_WORDS}]")
    for name, t, shape in (("cam_in", cam_in, (bs, cams)), ("active", active, (bs,)), ("cam_out", cam_out, (bs, cams)),
                           ("flags", flags, (bs, cams))):
        if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name} is a contiguous u8 {list(shape)} on the state's device")
    if cam_out is None:
        cam_out = torch.empty(bs, cams, dtype=torch.uint8, device=dev)
    if flags is None:
        flags = torch.empty(bs, cams, dtype=torch.uint8, device=dev)
    h, w = image_hw
    _lib.check(_lib.lib().simpb_camera_health_verdict(_ptr(cam_out), _ptr(flags), _ptr(state), _ptr(partials), _ptr(cam_in),
                                                      _ptr(active), params, bs, cams, int(h), int(w), _stream()),
               "simpb_camera_health_verdict")
    return cam_out, flags
