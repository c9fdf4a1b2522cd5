"""Frame runner: drives SimPB frame by frame for a fixed set of streams and replays the warm
(temporal) frame as ONE hipGraph.

Why: in eager mode a frame is ~1 700 kernel launches and the host, not the GPU, sets the pace. With
static shapes (a fixed-capacity 2D query set whose group table stays on the device, a temporal bank
in persistent buffers, a fixed-shape detection record) a frame has no host round trip inside it, so
it is captured once and replayed: per frame the host copies a few hundred bytes of metadata into
device buffers, launches the graph, and reads back two small records.

Frame 0 of a stream set has no history (a different dataflow) and runs eagerly; the first warm frame
runs eagerly too (lazy initialisation outside the capture), the second is captured. If a frame's 2D
query set ever exceeds the capacity, the overflow flags (read back with the records) trigger an eager
rerun of that frame with a larger capacity: the frame-end commit of the instance bank holds back when
a flag is set (csrc/bank.hip `hold`), so the rerun starts from the state the frame found, the graphs
are re-captured at the new capacity, and results never silently degrade. PipelinedRunner enqueues every
decoder one step early (before the previous frame's flags have reached the host) and therefore chains the
hold on the device: see its docstring.
"""
import contextlib
from dataclasses import dataclass

import numpy as np
import torch

from .plugin import routes
from .plugin.detection3d import SparseBox3DDecoder
from .results import POSE_KEYS, pose_row, world_tables


# Captures are taken in thread-local mode: with a process group initialised (one process per GPU, dist.py) the collective
# backend's watchdog thread polls events in the background, and in the default global mode a call of that kind from ANY thread
# invalidates a capture in progress. Everything a capture itself does happens on the capturing thread.
CAPTURE_MODE = "thread_local"


def stream_motion(metas, prev):
    """Per stream, what the bank needs to bring its cached anchors into this frame (instance_bank.py:90-97): T_temp2cur =
    inv(T_global of this frame) @ T_global of the stream's previous frame (f32 [bs, 4, 4]) and the time between the two
    (f32 [bs]). Host metadata only."""
    t = np.stack([np.asarray(m["T_global_inv"] @ p["T_global"], np.float32)
                  for m, p in zip(metas["img_metas"], prev["img_metas"])])
    dt = np.array([float(m["timestamp"] - p["timestamp"]) for m, p in zip(metas["img_metas"], prev["img_metas"])], np.float32)
    return t, dt


def refinement_time_step(dt, max_time_interval, default_time_interval):
    """The time step the refinement heads divide velocities by (instance_bank.py:87,108-113; csrc/bank.hip bank_get_kernel):
    the gap to the previous frame where it is usable (non-zero and within max_time_interval), the default otherwise. f32
    in, f32 out, compared in f32 like the kernel does."""
    dt = np.asarray(dt, np.float32)
    ok = (dt != 0) & (np.abs(dt) <= np.float32(max_time_interval))
    return np.where(ok, dt, np.float32(default_time_interval)).astype(np.float32)


def carry_inactive_metas(prev, metas, active):
    """The metas a frame is staged with when some streams of the batch sit it out. prev: dict(img_metas, projection_mat) as
    staged for the previous frame, i.e. every stream's LAST ACTIVE entries; metas: this frame's; active: one bool per stream.
    Returns a copy of `metas` in which an inactive stream's img_metas entry and projection_mat row are prev's. Staged against
    `prev` (stream_motion) such a stream gets dt = 0 and T_temp2cur = inv(T) @ T, and since the result is the next frame's
    `prev`, a stream that resumes measures its time step and ego-motion from its own last frame, not from the batch's last
    step. Pure host function: nothing of `prev` or `metas` is modified."""
    active = [bool(a) for a in active]
    if len(active) != len(metas["img_metas"]) or len(active) != len(prev["img_metas"]):
        raise ValueError(f"active has {len(active)} entries for {len(metas['img_metas'])} streams")
    out = dict(metas)
    out["img_metas"] = [m if a else p for a, m, p in zip(active, metas["img_metas"], prev["img_metas"])]
    proj = metas["projection_mat"].detach().cpu().clone()
    for i, a in enumerate(active):
        if not a:
            proj[i] = prev["projection_mat"][i]
    out["projection_mat"] = proj
    return out


def restart_metas(prev, metas, restart):
    """The `prev` a frame is staged against when some streams of the batch start over (step(..., restart=)). prev:
    dict(img_metas=...) of the frame before; metas: this frame's; restart: one bool per stream. Returns a copy of `prev` in
    which a restarted stream's img_metas entry is the stream's OWN current one: staged against it (stream_motion) the stream
    gets dt = 0 and T_temp2cur = inv(T) @ T, and the pose and time stamp of whoever held the slot before are never read --
    they may belong to another vehicle, in another global frame. Pure host function: nothing of `prev` or `metas` is modified."""
    restart = [bool(r) for r in restart]
    if len(restart) != len(metas["img_metas"]) or len(restart) != len(prev["img_metas"]):
        raise ValueError(f"restart has {len(restart)} entries for {len(metas['img_metas'])} streams")
    out = dict(prev)
    out["img_metas"] = [m if r else p for r, m, p in zip(restart, metas["img_metas"], prev["img_metas"])]
    return out


def normalise_restart(restart, num_streams, active=None, cold=False, independent=True, supported=True):
    """step / launch's `restart` -> None (no stream starts over: today's path) or a tuple of `num_streams` bools with a
    True. restart: None, or one bool per stream; active: None or the frame's activity mask; cold: the frame is the runner's
    first (every stream starts without history already: the flags are accepted and ignored); independent: the batch is a set
    of independent streams (a batch of one always is); supported: the runner can restart a stream at all. Pure host function."""
    if restart is None:
        return None
    flags = tuple(bool(r) for r in restart)
    if len(flags) != num_streams:
        raise ValueError(f"restart has {len(flags)} entries for {num_streams} streams")
    if not any(flags):
        return None
    if not supported:
        raise NotImplementedError("this runner cannot restart a stream: the single-frame part of the next frame is already in "
                                  "flight when a restart would have to take effect (use FrameRunner or PipelinedRunner)")
    if num_streams > 1 and not independent:
        raise ValueError("restarting a stream of a batch needs independent_streams=True (the reference's batch pads the "
                         "camera groups to the max over the batch: its streams are not independent)")
    if active is not None:
        if len(active) != num_streams:
            raise ValueError(f"active has {len(active)} entries for {num_streams} streams")
        both = [i for i, (r, a) in enumerate(zip(flags, active)) if r and not a]
        if both:
            raise ValueError(f"stream(s) {both} are paused and restarted in the same step: restart a stream in the step it resumes")
    return None if cold else flags


STATE_META_KEYS = ("T_global", "T_global_inv", "timestamp")   # what stream_motion reads of a previous frame's entry
_META_BYTES = (16 + 16 + 1) * 8


class StreamState:
    """One stream's temporal state, ready to go on in another slot, another runner or another process: the bank's stream
    record (include/simpb_hip.h; a u8 tensor on a device or on the host) and, of the img_metas entry of the stream's last
    ACTIVE frame -- the frame its bank rows belong to --, what stream_motion reads: T_global, T_global_inv (f64 [4, 4]) and
    timestamp (f64). `dims` = the record's (T, N, C, D), known on the host. export_stream of the runners makes one; `adopt=`
    of step / launch takes one. A state exported behind a frame still in flight (PipelinedRunner) is sealed when that frame's
    results are returned; touching it earlier raises RuntimeError."""

    def __init__(self, record, dims, T_global, T_global_inv, timestamp, sealed=True):
        from .plugin.instance_bank import record_layout
        self.dims = tuple(int(x) for x in dims)
        size = record_layout(*self.dims)["size"]
        if not torch.is_tensor(record) or record.dtype != torch.uint8 or record.dim() != 1 or record.numel() != size:
            raise ValueError(f"a stream record of (T, N, C, D) = {self.dims} is a u8 [{size}] tensor")
        self._record = record
        self.T_global = np.array(T_global, np.float64).reshape(4, 4)
        self.T_global_inv = np.array(T_global_inv, np.float64).reshape(4, 4)
        self.timestamp = float(timestamp)
        self._sealed = bool(sealed)
        self._ready = None      # event behind the launch that wrote the record last (None: nothing to wait for)

    @property
    def sealed(self):
        return self._sealed

    def _need_sealed(self):
        if not self._sealed:
            raise RuntimeError("this stream state was exported behind a frame whose results have not been returned yet: "
                               "collect() / step() / flush() the runner it came from first")

    @property
    def record(self):
        """The stream record (u8 tensor). On the device it may still be being written: order reads behind `wait(stream)`."""
        self._need_sealed()
        return self._record

    def wait(self, stream=None):
        """Order `stream` (None: the host) behind the launch that wrote the record."""
        self._need_sealed()
        if self._ready is not None:
            if stream is None:
                self._ready.synchronize()
            else:
                stream.wait_event(self._ready)

    def img_meta(self):
        """The img_metas entry of the stream's last active frame, reduced to STATE_META_KEYS."""
        return dict(T_global=self.T_global, T_global_inv=self.T_global_inv, timestamp=self.timestamp)

    def to(self, device):
        """The same state with its record on `device` (self if it is there already)."""
        device = torch.device(device)
        rec = self.record
        if rec.device == device or (rec.device.type == device.type == "cuda" and device.index is None):
            return self
        self.wait()
        return StreamState(rec.to(device), self.dims, self.T_global, self.T_global_inv, self.timestamp)

    def to_bytes(self):
        """One flat host byte string: the record, then T_global, T_global_inv and timestamp as little-endian f64."""
        self.wait()
        tail = np.concatenate([self.T_global.ravel(), self.T_global_inv.ravel(), [self.timestamp]]).astype("<f8")
        return self.record.cpu().numpy().tobytes() + tail.tobytes()

    @classmethod
    def from_bytes(cls, data):
        """The state `to_bytes` wrote (record on the host); a string that is not one is refused in words."""
        from .plugin.instance_bank import RECORD_HEADER, check_record, record_header
        data = bytes(data)
        if len(data) < RECORD_HEADER + _META_BYTES:
            raise ValueError(f"a stream state has at least {RECORD_HEADER + _META_BYTES} bytes; this string has {len(data)}")
        h = record_header(data)
        dims = (h["num_temp"], h["num_anchor"], h["embed_dims"], h["anchor_dims"])
        if min(dims) <= 0:
            raise ValueError(f"not a stream state: header sizes (T, N, C, D) = {dims}")
        body = data[:len(data) - _META_BYTES]
        check_record(body, *dims)
        tail = np.frombuffer(data[len(body):], "<f8")
        record = torch.from_numpy(np.frombuffer(body, np.uint8).copy())
        return cls(record, dims, tail[:16], tail[16:32], tail[32])


def adopt_metas(prev, adopt):
    """The `prev` a frame is staged against when some slots adopt a stream that ran elsewhere (step(..., adopt=)). prev:
    dict(img_metas=...) of the frame before; adopt: {slot: StreamState}. Returns a copy of `prev` in which an adopted slot's
    img_metas entry is the state's own (StreamState.img_meta): staged against it (stream_motion) the stream gets its own
    time step and ego-motion, and nothing of whoever held the slot before is read. Pure host function: nothing of `prev` or
    of the states is modified."""
    entries = list(prev["img_metas"])
    for slot, state in adopt.items():
        if not 0 <= int(slot) < len(entries):
            raise ValueError(f"adopt: slot {slot} of {len(entries)} streams")
        entries[int(slot)] = state.img_meta()
    out = dict(prev)
    out["img_metas"] = entries
    return out


def normalise_adopt(adopt, num_streams, dims, active=None, restart=None, independent=True, supported=True):
    """step / launch's `adopt` -> None (no slot adopts a stream: today's path) or a dict {slot: StreamState} in slot order.
    dims: the bank's (T, N, C, D); active / restart: the frame's masks as given (None or one bool per stream). Everything that
    can refuse an adoption does so here. Pure host function."""
    if adopt is None or len(adopt) == 0:
        return None
    if not supported:
        raise NotImplementedError("this runner cannot adopt a stream: the single-frame part of the next frame is already in "
                                  "flight when an adoption would have to take effect (use FrameRunner or PipelinedRunner)")
    if num_streams > 1 and not independent:
        raise ValueError("adopting a stream into a batch needs independent_streams=True (the reference's batch pads the "
                         "camera groups to the max over the batch: its streams are not independent)")
    out = {}
    for slot in sorted(adopt, key=int):
        state = adopt[slot]
        if int(slot) != slot or not 0 <= int(slot) < num_streams:
            raise ValueError(f"adopt: slot {slot!r} of {num_streams} streams")
        if not isinstance(state, StreamState):
            raise ValueError(f"adopt[{slot}] is a {type(state).__name__}, not a StreamState")
        state._need_sealed()
        if state.dims != tuple(dims):
            raise ValueError(f"adopt[{slot}]: stream record of a bank with (T, N, C, D) = {state.dims}; this bank has {tuple(dims)}")
        if active is not None and len(active) == num_streams and not active[int(slot)]:
            raise ValueError(f"stream {slot} is paused and adopted in the same step: adopt a stream in the step it runs")
        if restart is not None and len(restart) == num_streams and restart[int(slot)]:
            raise ValueError(f"stream {slot} is adopted and restarted in the same step: it either goes on or starts over")
        out[int(slot)] = state
    return out


def normalise_cameras(cameras, num_streams, num_cams, active=None):
    """step / launch's `cameras` -> None (every camera of every stream that takes part delivered a frame: today's path) or
    a tuple of `num_streams` tuples of `num_cams` bools with a False somewhere. cameras: None, or one sequence of num_cams
    bools per stream; active: None or one bool per stream. A paused stream's row is not looked at (it comes back all True:
    `active=False` overrides it); a stream that takes part with no camera at all is refused -- a stream without any frame is
    paused, not masked. Pure host function."""
    if cameras is None:
        return None
    rows = [tuple(bool(c) for c in row) for row in cameras]
    if len(rows) != num_streams:
        raise ValueError(f"cameras has {len(rows)} rows for {num_streams} streams")
    on = [True] * num_streams if active is None else [bool(a) for a in active]
    if len(on) != num_streams:
        raise ValueError(f"active has {len(on)} entries for {num_streams} streams")
    out = []
    for i, (row, a) in enumerate(zip(rows, on)):
        if len(row) != num_cams:
            raise ValueError(f"cameras[{i}] has {len(row)} entries for {num_cams} cameras")
        if not a:
            row = (True,) * num_cams
        elif not any(row):
            raise ValueError(f"stream {i} takes part with no valid camera: a stream without any frame is paused "
                             "(active=False), not masked")
        out.append(row)
    return None if all(all(row) for row in out) else tuple(out)


IDLE_IMAGES = ("compute", "skip")


def live_images(active, cameras, bs, cams):
    """The live-image table of a frame (include/simpb_hip.h): np.int32 [1 + bs * cams] with the number L of live images in
    front, their indices ascending behind it and zeros behind those. Image s * cams + c is live iff stream s is active and its
    camera c is valid. active / cameras: what normalise_active / normalise_cameras return -- None (all true), one bool per
    stream, one row of `cams` bools per stream; a paused stream's camera row is not looked at. Pure host function."""
    if active is not None and len(active) != bs:
        raise ValueError(f"active has {len(active)} entries for {bs} streams")
    if cameras is not None and (len(cameras) != bs or any(len(row) != cams for row in cameras)):
        raise ValueError(f"cameras is not {bs} rows of {cams} entries")
    live = [s * cams + c for s in range(bs) if active is None or active[s]
            for c in range(cams) if cameras is None or cameras[s][c]]
    table = np.zeros(1 + bs * cams, np.int32)
    table[0] = len(live)
    table[1:1 + len(live)] = live
    return table


class FrameInputs:
    """The per-frame decoder inputs of ONE frame in flight: a host buffer (pinned where the device is a GPU) and a device
    buffer for each, by name in `host` / `dev`:
        proj    f32 [bs, cams, 4, 4]  projection matrices
        t, dt   f32 [bs, 4, 4], [bs]  ego-motion T_temp2cur and time step to the stream's previous frame (stream_motion)
        ti      f32 [bs]              the refinement time step; only with time_step=(max_time_interval, default_time_interval)
        active  u8 [bs]               1: the stream takes part
        cam     u8 [bs, cams]         1: the camera delivered a frame
        pose    f64 [bs, 14]          results.pose_row per stream; only with pose=True
    and beside them `restart_host` / `restart_dev`, u8 [bs] (1: the stream starts over in this frame, restart_metas),
    which are filled, uploaded and named in `metas` only on a warm frame that restarts a stream.
    The device buffers are allocated here and never replaced: captured graphs bake their addresses in. `fill` is pure host
    work, `upload` the frame's copies to the device, `metas` the dict the head reads them through."""

    def __init__(self, bs, cams, device, time_step=None, pose=False):
        device = torch.device(device)
        self.time_step = time_step
        spec = dict(proj=((bs, cams, 4, 4), torch.float32, 0), t=((bs, 4, 4), torch.float32, 0), dt=((bs,), torch.float32, 0),
                    active=((bs,), torch.uint8, 1), cam=((bs, cams), torch.uint8, 1))
        if time_step is not None:
            spec["ti"] = ((bs,), torch.float32, 0)
        if pose:
            spec["pose"] = ((bs, 14), torch.float64, 0)
        self.host, self.dev = {}, {}
        for name, (shape, dtype, value) in spec.items():
            host = torch.full(shape, value, dtype=dtype)
            self.host[name] = host.pin_memory() if device.type == "cuda" else host
            self.dev[name] = torch.full(shape, value, dtype=dtype, device=device)
        host = torch.zeros(bs, dtype=torch.uint8)
        self.restart_host = host.pin_memory() if device.type == "cuda" else host
        self.restart_dev = torch.zeros(bs, dtype=torch.uint8, device=device)
        self.warm = self.masked = self.cam_masked = self.restarting = False   # of the frame last filled: what upload copies and metas names
        self.uploaded = None                # event: the host buffers have been copied to the device and may be refilled

    def fill(self, metas, prev, mask, cams, masked=False, cam_masked=False, restart=None):
        """One frame into the host buffers. metas: the frame's (paused streams already carried); prev: the metas of the
        frame before it (None: a cold frame, whose motion rows stay as they are); mask / cams: the frame's activity and
        camera masks (None: all ones); masked / cam_masked: the runner's graphs read the activity / camera buffer. A stream
        whose img_metas entry lacks results.POSE_KEYS (a paused one) keeps the pose row it had. restart: None or one bool
        per stream with a True (normalise_restart); on a warm frame those streams' motion is staged against their own
        metas (restart_metas) and the flags go to the head."""
        if self.uploaded is not None:
            self.uploaded.synchronize()     # the previous frame's copies out of these buffers (long done in practice)
        h = self.host
        proj = metas["projection_mat"]
        h["proj"].copy_(proj.cpu() if proj.is_cuda else proj)
        self.warm, self.masked, self.cam_masked = prev is not None, masked, cam_masked
        self.restarting = self.warm and restart is not None
        if self.restarting:
            prev = restart_metas(prev, metas, restart)
            self.restart_host.numpy()[:] = restart
        if self.warm:
            t, dt = stream_motion(metas, prev)
            h["t"].copy_(torch.from_numpy(t))
            h["dt"].copy_(torch.from_numpy(dt))
        if "ti" in h:
            # the time step the refinement heads divide by (instance_bank.py:108-113, csrc/bank.hip bank_get_kernel): the
            # frame gap where it is usable, the default otherwise -- a function of the time stamps alone, in f32 like there
            max_dt, default = self.time_step
            h["ti"].numpy()[:] = refinement_time_step(dt, max_dt, default) if self.warm else np.float32(default)
        h["active"].numpy()[:] = 1 if mask is None else mask
        h["cam"].numpy()[:] = 1 if cams is None else cams
        if "pose" in h:
            rows = h["pose"].numpy()
            for i, m in enumerate(metas["img_metas"]):
                if all(k in m for k in POSE_KEYS):
                    rows[i] = pose_row(m)

    def upload(self, stream):
        """The filled frame's host-to-device copies, on `stream`: the projection matrices, time step and pose always, motion
        for a warm frame, a mask once the runner's graphs read it."""
        live = dict(proj=True, ti=True, pose=True, active=self.masked, cam=self.cam_masked, t=self.warm, dt=self.warm)
        with torch.cuda.stream(stream):
            for name, dev in self.dev.items():
                if live[name]:
                    dev.copy_(self.host[name], non_blocking=True)
            if self.restarting:
                self.restart_dev.copy_(self.restart_host, non_blocking=True)
            self.uploaded = torch.cuda.Event()
            self.uploaded.record(stream)

    def metas(self, img_metas, wh, wh_host):
        """The metas dict the head reads the filled frame through (its overflow key is the runner's to add)."""
        d = self.dev
        out = dict(projection_mat=d["proj"], image_wh=wh, image_wh_host=wh_host, img_metas=img_metas)
        if self.warm:
            out["bank_inputs"] = (d["t"], d["dt"])
        if self.masked:
            out["active"] = d["active"]
        if self.cam_masked:
            out["camera_valid"] = d["cam"]
        if "ti" in d:
            out["time_interval"] = d["ti"]
        if self.restarting:
            out["restart"] = self.restart_dev
        return out


class FrameRunner:
    # a frame's inputs are staged while the frame before it still reads its own (SplitPipelinedRunner: part A(t) runs
    # beside part B(t-1)): one FrameInputs per feature slot, with the refinement time step that part A needs staged
    SLOT_INPUTS = False

    def __init__(self, model, batch_size, image_hw, capacity=1536, device=None, use_graph=True, independent_streams=False,
                 raw_input=None, img_norm_cfg=None, world_output=None, raw_format="bgr", raw_colour="jfif",
                 raw_layout=None, raw_surfaces=False, raw_rig=None, idle_images="compute", camera_health=None, raw_roll=None,
                 raw_chroma=None):
        """independent_streams: the batch is a set of independent camera streams, each decoded exactly as a batch of one
        would be (`capacity` 2D slots per stream; SimPBHead.independent_streams) -- the throughput form of BASELINE config
        #3. False: the reference's batch semantics (camera groups padded to the max over the batch).

        raw_input=(Hs, Ws): frames arrive as the decoder's u8 [bs, cams, Hs, Ws, 3] (device or pinned host memory) and the
        reference's resize / crop / flip / normalise (img_norm_cfg, default: the shipped configs') runs on the device as the
        first launches of the frame (csrc/preprocess.hip), keyed by the frame's own aug_config: see _ensure_plan.
        raw_format="nv12" | "nv21", raw_colour="jfif" | "bt601" | "bt709" (with raw_input only): the frames are 4:2:0
        semi-planar YCbCr, u8 [bs, cams, Hs * 3 / 2, Ws] (preprocess.ResamplePlan has the layout), converted to BGR inside the
        ingest's first launch. The default "bgr" is the packed form above. "p010": the 10-bit form of NV12, u8 [bs, cams,
        Hs * 3 / 2, Ws * 2] (raw_colour "bt601" or "bt709"). "yuv420p" / "yvu420p" (a software decoder's planar I420 / YV12): u8
        [bs, cams, Hs * 3 / 2, Ws], three planes. "yuyv" / "uyvy" (packed 4:2:2, a camera without a codec): u8 [bs, cams, Hs, Ws, 2].
        "rgb": u8 [bs, cams, Hs, Ws, 3], R first. "bgra" / "rgba": u8 [bs, cams, Hs, Ws, 4], byte 3 ignored; raw_colour says nothing
        about the last three (preprocess.ResamplePlan has every layout).
        raw_layout=preprocess.SurfaceLayout or a dict of its keyword arguments (with raw_input only): every image is a decoder
        surface with a padded pitch / plane height / chroma offset; frames are then u8 [bs, cams, image_bytes].
        raw_surfaces=True (with raw_input only, with or without raw_layout): `img` is a nested list [bs][cams] of device u8
        tensors, one surface each, read where they lie: there is no staging buffer and no frame copy, only a table of
        bs * cams addresses per frame. A surface stays valid and unchanged until the results of its frame have been returned
        (step's return, the collect that yields the frame, or flush); the runner holds a reference to each until then. A
        paused stream or a masked camera takes None in place of a tensor.
        raw_rig=[preprocess.CameraSource, ...], one per camera of the model (instead of raw_input and everything that goes with
        it): the cameras differ in source size, format, colour standard, layout, resize, crop or flip and give the runner's
        image size. `img` is the nested list [bs][cams] of raw_surfaces, with the same lifetime rule; a None (paused stream,
        masked camera) is an image the ingest skips. metas["img_metas"][0]["aug_config"] is not read: the ingest and the 2D
        record both follow the rig (preprocess.RigPlan); `set_raw_rig` changes it between frames.
        raw_roll=degrees | [degrees per camera] (with raw_input only; every raw_format, raw_layout and raw_surfaces): the cameras'
        mount roll, positive counter-clockwise on screen -- the reference's `img.rotate` behind resize, crop and flip, done inside
        the ingest's second launch with Pillow's bytes (preprocess.ResamplePlan has the rule). It is a property of the mount, not
        of the frame: the aug_config's own `rotate` stays refused. With raw_rig each CameraSource brings its own `roll`. The 2D
        records are unchanged: the reference's decode_box2d does not look at rotate. camera_health sees the rolled image, black
        corners included. None, or rolls that are all multiples of 360: nothing of this is launched.
        raw_chroma="replicate" | "jpeg" (with raw_input only; raw_format nv12, nv21, yuv420p, yvu420p, yuyv or uyvy, in every
        raw_layout, with raw_surfaces and with raw_roll): "jpeg" interpolates the subsampled chroma as libjpeg's decoder does at
        its defaults, inside the ingest's first launch; with raw_colour="jpeg" (libjpeg's own colour constants, also taken by
        "yuv444p" frames) the native planes of a JPEG give the bytes the reference's loader would have decoded from that file
        (preprocess.ResamplePlan has the rule and says what is pinned to libjpeg). With raw_rig each CameraSource brings its own
        `chroma`. camera_health, the 2D records and the decoder see nothing new. None or "replicate": nothing changes.

        world_output=dict(classes=..., tracking=bool, threshold=float | None): a second output per frame, the WORLD RECORD
        (csrc/world.hip, results.py): boxes in the global frame, threshold and class ranges applied, kept rows packed, a
        row count per stream -- one more launch at the end of the decoder, inside its graph. Each stream's img_metas entry
        must then carry results.POSE_KEYS. None (default): nothing of this exists.

        idle_images="compute" | "skip": what the backbone does with the image of a paused stream (step's `active`) or of a
        camera that delivered nothing (`cameras`). "compute" (default): it runs on every image slot, as ever. "skip": from the
        first frame with such an image on, every frame stages its live-image table (live_images) with the images, and the
        backbone's convolutions walk the live images only (the *_live entry points of include/simpb_hip.h): the rest is
        neither read nor written. Results are the same bits for every stream that takes part. Until that first frame
        nothing is staged and the graphs are the ordinary ones; that frame drops every graph once (stats["image_skip"]
        counts the frames staged with a table, an all-live frame with the full one).

        camera_health=health.CameraHealth (or a dict of its keywords; raw frames only: raw_input or raw_rig): every frame gets
        two more launches right behind the ingest, on its stream and inside its graph (csrc/health.hip): integer statistics of
        every image, then a verdict per camera -- dark, bright, flat (a covered lens), frozen (the same pixels again),
        non-finite -- that writes the camera mask the decoder of this very frame reads, ANDed with the host's `cameras` /
        `active`. A faulty camera is decoded as a missing one (step's `cameras`); if every camera of a stream is faulty none is
        dropped (fail open). The runner is camera-masked from construction, one captured graph serves every verdict, and the
        frozen check's state advances once per ingested frame (a re-run after a 2D overflow re-reads the verdict). The flags
        (health.DARK ...) come back with the records: res[s]["img_bbox"]["camera_health"] (u8 [cams]), `last_health`,
        stats["health_dropped"], and `health_state()`. With act=False they are reported and nothing is dropped. With
        idle_images="skip" a camera the device drops is still computed by the backbone: the host cannot know of it before it
        enqueues the frame. None (default): nothing of this is allocated, staged or launched."""
        if idle_images not in IDLE_IMAGES:
            raise ValueError(f"idle_images={idle_images!r}: one of {IDLE_IMAGES}")
        self.idle_images = idle_images
        self.raw_roll = 0.0                 # raw_roll=: one roll for every camera, or a tuple of one per camera (degrees)
        if raw_roll is not None:
            from .preprocess import check_roll
            if raw_rig is not None:
                raise ValueError("raw_rig describes every camera by itself: each CameraSource brings its own roll=, raw_roll must not "
                                 "be given with it")
            if raw_input is None:
                raise ValueError("raw_roll describes raw frames: it needs raw_input=(Hs, Ws)")
            if isinstance(raw_roll, (list, tuple)):
                if len(raw_roll) != model.head.num_cams:
                    raise ValueError(f"raw_roll lists {len(raw_roll)} rolls, the model has {model.head.num_cams} cameras")
                self.raw_roll = tuple(check_roll(r) for r in raw_roll)
            else:
                self.raw_roll = check_roll(raw_roll)
        self.raw_chroma = "replicate"       # raw_chroma=: how subsampled chroma becomes a Cb / Cr per pixel ("replicate" | "jpeg")
        if raw_chroma is not None:
            if raw_rig is not None:
                raise ValueError("raw_rig describes every camera by itself: each CameraSource brings its own chroma=, raw_chroma must "
                                 "not be given with it")
            if raw_input is None:
                raise ValueError("raw_chroma describes raw frames: it needs raw_input=(Hs, Ws)")
            self.raw_chroma = raw_chroma    # (an unknown mode, or a format that does not take it, is refused with the format below)
        self.skipping = False               # True from the first frame with a dead image on (idle_images="skip"): the backbone reads live_dev
        self.live_pin = self.live_dev = None    # per feature slot: the live-image table, pinned host side and fixed device side
        self.live_staged = None             # per feature slot: event behind the slot's last copy out of its pinned table
        self.health = None                  # health.CameraHealth (camera_health=); None: nothing of it exists
        self.health_slots = None            # per feature slot: partial rows, cam_eff, flags and the staged host masks
        self.health_dev_state = None        # the frozen check's state, one per runner: int64 [bs, cams, 2]
        self.last_health = None             # flags u8 [bs, cams] (numpy) of the frame last returned
        self.health_hold = False            # True while a frame is re-run: its verdict stands, the state does not advance again
        if camera_health is not None:
            from .health import CameraHealth
            if raw_input is None and raw_rig is None:
                raise ValueError("camera_health looks at the images the device ingest writes: it needs raw frames (raw_input= or "
                                 "raw_rig=), not tensor input")
            self.health = CameraHealth.make(camera_health)
        self.model = model
        self.head = model.head
        self.bs = batch_size
        self.independent = bool(independent_streams) and batch_size > 1
        if self.independent:   # (before anything is allocated: the allocation launch would refuse the first frame)
            from .plugin.allocation import check_stream_groups
            check_stream_groups(batch_size, self.head.num_cams)
        self.head.independent_streams = self.independent
        self.capacity = int(capacity)
        self.use_graph = use_graph
        self.device = device if device is not None else next(model.parameters()).device
        h, w = image_hw
        dev = self.device
        cams = self.head.num_cams
        self.image_hw = (int(h), int(w))
        self.raw_input = (int(raw_input[0]), int(raw_input[1])) if raw_input is not None else None
        self.img_norm_cfg = img_norm_cfg
        self.plan = None                    # preprocess.ResamplePlan of the stream's aug_config (raw_input mode)
        self.raw_format, self.raw_colour = raw_format, raw_colour
        self.raw_layout = None              # preprocess.SurfaceLayout of every image (raw_layout=; None: the tight form)
        self.surfaces = bool(raw_surfaces)  # img is a nested list of device tensors; self.raw is then the int64 address table
        self.pin_table = None               # raw_surfaces: the pinned host side of that table
        self.rig = None                     # raw_rig: the cameras' preprocess.CameraSource; self.plan is then their RigPlan
        if raw_rig is not None:
            if raw_input is not None or (raw_format, raw_colour) != ("bgr", "jfif") or raw_layout is not None or raw_surfaces:
                raise ValueError("raw_rig describes every camera by itself: raw_input / raw_format / raw_colour / raw_layout / "
                                 "raw_surfaces must not be given with it")
            self.img, self.surfaces = None, True
            self.plan = self._rig_plan(raw_rig)
            self.rig = self.plan.sources
            self.raw = self._raw_buffer()
            self.pin_table = torch.zeros(batch_size, cams, dtype=torch.int64).pin_memory()
        elif self.raw_input is None:
            if (raw_format, raw_colour) != ("bgr", "jfif"):
                raise ValueError(f"raw_format={raw_format!r} / raw_colour={raw_colour!r} describe raw frames: they need raw_input=(Hs, Ws)")
            if raw_layout is not None or raw_surfaces:
                raise ValueError("raw_layout / raw_surfaces describe raw frames: they need raw_input=(Hs, Ws)")
            self.img, self.raw = torch.zeros(batch_size, cams, 3, h, w, device=dev), None
        else:   # (no fp32 staging buffer in this mode)
            from .preprocess import SurfaceLayout, frame_shape, plan_key
            # (an unknown format, standard or chroma mode is refused here)
            plan_key(self.raw_input, None, raw_format, raw_colour, None, self.raw_roll, self.raw_chroma)
            self.img = None
            if raw_layout is not None:
                self.raw_layout = SurfaceLayout.make(raw_layout, self.raw_input, raw_format)
            self.raw = self._raw_buffer()
            if self.surfaces:   # (FrameRunner: one pinned table; its copy is over when step returns)
                self.pin_table = torch.zeros(batch_size, cams, dtype=torch.int64).pin_memory()
        self.wh = torch.tensor([float(w), float(h)], device=dev).view(1, 1, 2).repeat(batch_size, cams, 1)
        self.wh_host = (int(w), int(h))
        # per-stream activity (step(..., active=)) and per-camera validity (step(..., cameras=)): uploaded and handed to the
        # head once a caller has paused a stream / dropped a camera; until then the head is called without them (see
        # _activity, _camera_mask)
        self.masked = False                 # True from the first frame with a paused stream on: the graphs read `active`
        self.last_active = (True,) * batch_size   # mask of the frame last returned
        self.cam_masked = False             # True from the first frame with a missing camera on: the graphs read `cam`
        if self.health is not None:
            self._health_setup()
        bank = self.head.instance_bank
        time_step = (bank.max_time_interval, bank.default_time_interval) if self.SLOT_INPUTS else None
        self.slot_inputs = [FrameInputs(batch_size, cams, dev, time_step, pose=world_output is not None)
                            for _ in range(2 if self.SLOT_INPUTS else 1)]
        self.inputs = self.slot_inputs[0]   # the set last filled
        bank.enable_static(batch_size, dev)
        self.head.static_capacity = self.capacity
        self.prev_metas = None
        self.graph = None
        self.outputs = None
        # the graph of a frame that restarts a stream (step(..., restart=)): the same frame with metas["restart"] read by the
        # head. Captured at the first warm frame with a True, replayed on such frames only, dropped with the ordinary one
        self.restart_graph = None
        self.restart_outputs = None
        self.warm_frames = 0
        self.host3d = self.host2d = self.host_flag = None
        self.stats = dict(eager=0, replay=0, overflow=0)   # (+ "restart": frames that restarted a stream, from the first one on)
        if self.health is not None:
            self.stats["health_dropped"] = 0   # cameras the verdict took out of a frame, summed over the frames returned
        self.decoded = [False] * batch_size   # per slot: it has taken part in a frame here (export_stream needs that)
        self.last_rec3d = None      # device record f32 [bs, num_output, 15] of the frame last returned (dist.DetectionGather)
        self.last_rec2d = None      # ... and its 2D record f32 [bs, capacity, 8]
        # event after which those records may be overwritten (set by their consumer, if any). The records of a replayed
        # frame live in graph memory: EVERY graph of this runner that may write that memory waits for it before its next
        # replay (the decoder graphs and, in SplitPipelinedRunner, part A, which shares the pool of part B)
        self.rec_consumed = None
        self.world_output = None
        if world_output is not None:
            tracking = bool(world_output.get("tracking", False))
            self.world_output = dict(classes=tuple(world_output["classes"]), tracking=tracking,
                                     threshold=world_output.get("threshold"),
                                     tables=world_tables(world_output["classes"], tracking))
            self.host_world = self.host_count = None
            self.last_world = None          # device world record f64 [bs, num_output, 16] of the frame last returned ...
            self.last_world_count = None    # ... and its row counts i32 [bs] (-1: the stream was paused); as last_rec3d

    # ------------------------------------------------------------------ per-frame host work
    def _check_pose(self, metas, mask):
        """world_output: every stream that takes part brings its pose (checked before anything is enqueued)."""
        if self.world_output is None:
            return
        for i, m in enumerate(metas["img_metas"]):
            missing = [k for k in POSE_KEYS if k not in m]
            if missing and (mask is None or mask[i]):
                raise ValueError(f"world_output: img_metas[{i}] lacks {missing}")

    def _records(self, outs, aug_config, inputs):
        """The record tail of a frame whose per-frame inputs are `inputs`: the head's outputs -> the frame's record tuple
        (every tensor of a fixed shape); with world_output the world record's launch behind it (the last node of the frame)
        and its two tensors at the end of the tuple."""
        rec3d, rec2d = self.head.decoder.decode_static_device(
            outs["classification"], outs["prediction"], outs["instance_id"], outs["quality"],
            outs["classification2d"], outs["prediction2d"], outs["alloc_list"][-1], aug_config)
        if self.world_output is None:
            return rec3d, rec2d, outs["overflow"]
        cfg = self.world_output
        world, count = self.head.decoder.world_record(rec3d, inputs.dev["pose"], inputs.dev["active"] if self.masked else None,
                                                      cfg["tables"], cfg["threshold"])
        return rec3d, rec2d, outs["overflow"], world, count

    def _raw_buffer(self):
        """The device buffer the ingest reads: the frames' staging buffer, or with raw_surfaces the table of their addresses."""
        from .preprocess import frame_shape
        cams = self.head.num_cams
        if self.surfaces:
            return torch.zeros(self.bs, cams, dtype=torch.int64, device=self.device)
        shape = (frame_shape(self.raw_input, self.raw_format) if self.raw_layout is None or self.raw_layout.tight
                 else (self.raw_layout.image_bytes,))
        return torch.zeros(self.bs, cams, *shape, dtype=torch.uint8, device=self.device)

    def set_raw_layout(self, raw_layout):
        """The decoder's surfaces change their layout (raw_layout as in the constructor; None: the tight form) from the next
        frame on: a changed layout is a changed plan key, so every graph is dropped and the staging buffers are made anew.
        A pipelined runner takes the change between frames only: with a frame still in flight it is refused (`flush()` first)."""
        from .preprocess import SurfaceLayout
        if self.raw_input is None:
            raise ValueError("raw_layout describes raw frames: it needs raw_input=(Hs, Ws)")
        if self._in_flight():
            raise RuntimeError(f"set_raw_layout with {self._in_flight()} frame(s) in flight: flush() the runner first (their results "
                               "have not been returned, and the buffers they were staged in would be replaced)")
        new = None if raw_layout is None else SurfaceLayout.make(raw_layout, self.raw_input, self.raw_format)
        if (new.key if new is not None else None) == (self.raw_layout.key if self.raw_layout is not None else None):
            return
        torch.cuda.synchronize(self.device)   # nothing in flight reads the old buffers
        self._drop_all_graphs()
        self.raw_layout, self.plan = new, None
        self._new_raw_buffers()

    def _new_raw_buffers(self):
        self.raw = self._raw_buffer()

    def _rig_plan(self, sources):
        """raw_rig: the RigPlan of `sources`, refused unless it has one camera per camera of the model and the runner's size."""
        from .preprocess import RigPlan
        sources = list(sources)
        if len(sources) != self.head.num_cams:
            raise ValueError(f"raw_rig has {len(sources)} cameras, the model {self.head.num_cams}")
        plan = RigPlan(sources, self.img_norm_cfg)
        if plan.out_hw != self.image_hw:
            raise ValueError(f"raw_rig turns its frames into {plan.out_hw} images; this runner was built for {self.image_hw}")
        return plan

    def set_raw_rig(self, sources):
        """The rig changes (a camera was replaced, a decoder reconfigured) from the next frame on, by set_raw_layout's rules:
        refused with frames in flight, nothing happens for an equal key, otherwise every graph is dropped (they hold the old
        rig by value and the old tables' addresses) and the plan is made anew."""
        if self.rig is None:
            raise ValueError("set_raw_rig changes the rig of a raw_rig runner")
        if self._in_flight():
            raise RuntimeError(f"set_raw_rig with {self._in_flight()} frame(s) in flight: flush() the runner first (their results "
                               "have not been returned)")
        plan = self._rig_plan(sources)
        if plan.key == self.plan.key:
            return
        torch.cuda.synchronize(self.device)   # nothing in flight reads the old tables
        self._drop_all_graphs()
        self.plan, self.rig = plan, plan.sources

    def _aug(self, metas):
        """What the decoder maps its 2D boxes back to source pixels with: the frame's aug_config, or with raw_rig the rig's
        plan (its per-camera table)."""
        return self.plan if self.rig is not None else metas["img_metas"][0]["aug_config"]

    def _in_flight(self):
        """Frames fed whose results have not been returned (a step of this runner returns its own frame's)."""
        return 0

    def _ensure_plan(self, metas):
        """raw_input mode: the ingest tables follow the frame's aug_config (metas["img_metas"][0], the dict the decoder reads
        as well). A frame whose (source size, resize_dims, crop, flip, format, colour) differ from the resident plan's gets a
        new plan, and every captured graph is dropped first (they bake the old tables' addresses and the decoder's crop /
        resize in): a frame never runs on stale tables."""
        from .preprocess import ResamplePlan, plan_key
        if self.rig is not None:   # (the rig's plan does not follow the metas; reserve allocates on the first frame only)
            self.plan.reserve(self.bs * self.head.num_cams, self.device)
            return
        aug = metas["img_metas"][0]["aug_config"]
        if self.plan is not None and self.plan.key == plan_key(self.raw_input, aug, self.raw_format, self.raw_colour, self.raw_layout,
                                                               self.raw_roll, self.raw_chroma):
            return
        plan = ResamplePlan(self.raw_input, aug, self.img_norm_cfg, self.raw_format, self.raw_colour, self.raw_layout, self.raw_roll,
                            self.raw_chroma)
        if plan.out_hw != self.image_hw:
            raise ValueError(f"aug_config {aug} turns {self.raw_input} frames into {plan.out_hw} images; this runner was built for "
                             f"{self.image_hw}")
        if self.plan is not None:
            torch.cuda.synchronize(self.device)   # nothing in flight reads the old tables
            self._drop_all_graphs()
        self.plan = plan.reserve(self.bs * self.head.num_cams, self.device)

    def _check_frames(self, img, mask=None, cams=None):
        """The frames of a step as `_stage_frames` takes them; a wrong form is refused before anything is enqueued."""
        if self.surfaces:
            return self._check_surfaces(img, mask, cams)
        if not torch.is_tensor(img) or img.dtype != torch.uint8 or tuple(img.shape) != tuple(self.raw.shape):
            what = " frames" if self.raw_format == "bgr" else f" {self.raw_format} frames"
            if self.raw_layout is not None and not self.raw_layout.tight:
                what = f" images, each a {self.raw_layout.describe()}"
            got = f"{img.dtype} {tuple(img.shape)}" if torch.is_tensor(img) else type(img).__name__
            raise ValueError(f"raw_input runner takes u8 {tuple(self.raw.shape)}{what}, got {got}")
        return img

    def _check_surfaces(self, img, mask, cams):
        """raw_surfaces: img [bs][cams] of device u8 tensors -> (addresses [bs][cams], the tensors). None stands for the surface
        of a paused stream or a masked camera (a paused stream's whole row may be None); its table entry is another surface of
        the same step: the kernel runs on every slot, and what it makes of that one is never looked at."""
        from .preprocess import SurfaceLayout, check_surfaces
        num_cams = self.head.num_cams
        if torch.is_tensor(img) or not isinstance(img, (list, tuple)) or len(img) != self.bs:
            raise ValueError(f"raw_surfaces runner takes a nested list [{self.bs}][{num_cams}] of device u8 tensors, one surface each "
                             f"(got {type(img).__name__})")
        rows, held = [], []
        for i, row in enumerate(img):
            paused = mask is not None and not mask[i]
            if row is None and paused:
                row = [None] * num_cams
            if not isinstance(row, (list, tuple)) or len(row) != num_cams:
                raise ValueError(f"raw_surfaces: stream {i} brings {num_cams} surfaces, one per camera")
            for c, t in enumerate(row):
                if t is None and not (paused or (cams is not None and not cams[i][c])):
                    raise ValueError(f"raw_surfaces: stream {i} camera {c} has no surface, and is neither paused nor masked")
            rows.append(list(row))
            held += [t for t in row if t is not None]
        if self.rig is not None:   # each surface against its own camera's layout; a None is address 0: the ingest skips it
            ptrs, device = self.plan.surface_table([t for row in rows for t in row])
            if device != torch.device(self.raw.device):
                raise ValueError(f"raw_rig: the surfaces are on {device}, the runner on {self.raw.device}")
            n = num_cams
            return [ptrs[i * n:(i + 1) * n] for i in range(self.bs)], held
        if not held:
            raise ValueError("raw_surfaces: this step brings no surface at all (every camera of every active stream is masked): "
                             "the address table needs one live surface")
        layout = self.raw_layout if self.raw_layout is not None else SurfaceLayout(self.raw_input, self.raw_format)
        if check_surfaces(held, layout) != torch.device(self.raw.device):
            raise ValueError(f"raw_surfaces: the surfaces are on {held[0].device}, the runner on {self.raw.device}")
        spare = held[0].data_ptr()
        return [[spare if t is None else t.data_ptr() for t in row] for row in rows], held

    def _stage_frames(self, dst, frames, pin=None):
        """This frame's images into the buffer the ingest reads (on the current stream): the frames themselves, or with
        raw_surfaces their bs * cams addresses through the pinned table `pin` -- the surfaces are not copied."""
        if not self.surfaces:
            dst.copy_(frames, non_blocking=True)
            return
        pin.copy_(torch.tensor(frames[0], dtype=torch.int64))
        dst.copy_(pin, non_blocking=True)

    def _extract(self, img, raw, slot=0):
        extra = dict(live=self.live_dev[slot]) if self.skipping else {}
        launches = self._health_launches(slot)
        if launches is not None:
            extra["on_ingest"] = launches
        return self.model.extract_feat(raw, raw_plan=self.plan, **extra) if raw is not None else self.model.extract_feat(img, **extra)

    FEATURE_SLOTS = 1

    def _idle(self, mask, cams):
        """idle_images="skip": the frame's live-image table (host), or None while no frame has had a dead image. The first
        frame that has one switches the runner over, before anything of it is enqueued: every graph is dropped once (the
        backbone's, and the decoder's bound to them) and the tables get their pinned host side and their device address."""
        if self.idle_images != "skip" or (not self.skipping and mask is None and cams is None):
            return None
        if not self.skipping:
            torch.cuda.synchronize(self.device)   # nothing in flight replays a backbone graph that does not read the table
            self._drop_all_graphs()
            n = 1 + self.bs * self.head.num_cams
            self.live_pin = [torch.zeros(n, dtype=torch.int32).pin_memory() for _ in range(self.FEATURE_SLOTS)]
            self.live_dev = [torch.zeros(n, dtype=torch.int32, device=self.device) for _ in range(self.FEATURE_SLOTS)]
            self.live_staged = [None] * self.FEATURE_SLOTS
            self.skipping = True
        self.stats["image_skip"] = self.stats.get("image_skip", 0) + 1
        return live_images(mask, cams, self.bs, self.head.num_cams)

    def _stage_live(self, slot, table):
        """The frame's live-image table into the slot's device buffer, on the current stream -- the one the slot's images are
        staged on and its backbone runs on, in front of both."""
        if table is None:
            return
        if self.live_staged[slot] is not None:
            self.live_staged[slot].synchronize()   # the slot's last copy out of its pinned table (long done)
        self.live_pin[slot].numpy()[:] = table
        self.live_dev[slot].copy_(self.live_pin[slot], non_blocking=True)
        self.live_staged[slot] = torch.cuda.Event()
        self.live_staged[slot].record(torch.cuda.current_stream())

    # ------------------------------------------------------------------ camera health
    def _health_setup(self):
        """camera_health: the buffers of every feature slot and the one state. The graphs read the slot's cam_eff in place
        of the host's mask from the first frame on (all ones until a camera is dropped)."""
        from . import health as H
        dev, bs, cams = self.device, self.bs, self.head.num_cams
        h, w = self.image_hw
        self.health_params = self.health.params(self.img_norm_cfg)
        words = H.partials_bytes(bs * cams, h, w) // 8
        pin = lambda t: t.pin_memory() if torch.device(dev).type == "cuda" else t   # noqa: E731
        self.health_slots = [dict(partials=torch.zeros(words, dtype=torch.int64, device=dev),
                                  cam_eff=torch.ones(bs, cams, dtype=torch.uint8, device=dev),
                                  flags=torch.zeros(bs, cams, dtype=torch.uint8, device=dev),
                                  masks_pin=pin(torch.ones(bs + bs * cams, dtype=torch.uint8)),   # active | cam, the host's
                                  masks=torch.ones(bs + bs * cams, dtype=torch.uint8, device=dev),
                                  staged=None, host=pin(torch.zeros(bs, cams, dtype=torch.uint8)))
                             for _ in range(self.FEATURE_SLOTS)]
        self.health_dev_state = H.new_state(bs, cams, dev)
        self.cam_masked = True

    def _stage_health(self, slot, mask, cams):
        """The host's `active` and `cameras` rows for the slot's verdict, on the current stream -- the one the slot's images
        are staged on and its ingest runs on (as _stage_live; not with the decoder's FrameInputs, which travel on another)."""
        if self.health is None:
            return
        hs = self.health_slots[slot]
        if hs["staged"] is not None:
            hs["staged"].synchronize()   # the slot's last copy out of its pinned rows (long done)
        rows = hs["masks_pin"].numpy()
        rows[:self.bs] = 1 if mask is None else mask
        rows[self.bs:] = 1 if cams is None else np.asarray(cams, np.uint8).reshape(-1)
        hs["masks"].copy_(hs["masks_pin"], non_blocking=True)
        hs["staged"] = torch.cuda.Event()
        hs["staged"].record(torch.cuda.current_stream())

    def _health_launches(self, slot):
        """The callable extract_feat runs right behind the ingest (None: no camera health, or a re-run of the frame)."""
        if self.health is None or self.health_hold:
            return None
        from . import health as H
        hs, bs, cams = self.health_slots[slot], self.bs, self.head.num_cams

        def launches(images):
            H.image_health_stats(images, out=hs["partials"])
            H.camera_health_verdict(hs["partials"], self.health_dev_state, self.health_params, self.image_hw,
                                    cam_in=hs["masks"][bs:].view(bs, cams), active=hs["masks"][:bs],
                                    cam_out=hs["cam_eff"], flags=hs["flags"])
        return launches

    def health_state(self):
        """camera_health: a host copy of the frozen check's state behind everything enqueued so far: dict(prev_hash u64,
        repeats u32, frames u32), each [bs, cams] -- `frames` counts the frames a camera took part in."""
        if self.health is None:
            raise ValueError("health_state: this runner was built without camera_health")
        from .health import state_to_host
        torch.cuda.synchronize(self.device)
        return state_to_host(self.health_dev_state)

    def _health_results(self, results, flags):
        """The frame's flags (host u8 [bs, cams]) into its results, last_health and stats["health_dropped"]."""
        from .health import FAIL_OPEN, FAULTS
        flags = flags.numpy().copy()
        self.last_health = flags
        if self.health.act:
            dropped = ((flags & FAULTS) != 0) & ((flags & FAIL_OPEN) == 0)
            self.stats["health_dropped"] = self.stats.get("health_dropped", 0) + int(dropped.sum())
        for i, res in enumerate(results):
            if res is not None:
                res["img_bbox"]["camera_health"] = flags[i]
        return results

    # A frame that is captured and replayed exposes nothing but its records, so it computes nothing else (routes.lean_tokens,
    # routes.lean_refine2d; profiles/lean_frames.md). Both act for the length of a capture only: eager frames (use_graph=False,
    # the frames before a capture, force_eager, re-runs) and direct calls of the model keep every output they have.
    @contextlib.contextmanager
    def _capturing(self):
        """Around a capture that runs backbone + FPN: the FPN's output convolutions write the f16 token rows alone, so the
        captured frame's feature_maps[0] is the f16 tensor and its graph pool holds no fp32 rows. Needs the routes on which
        every reader of the tokens takes f16 rows; restored on the way out, also after an exception."""
        R = routes.R
        neck = getattr(self.model, "img_neck", None)
        on = (neck is not None and R.lean_tokens and R.dense and R.fused_dfa and (R.msda_linear or R.split_value_proj))
        if not on:
            yield
            return
        before = getattr(neck, "f16_tokens_only", False)
        neck.f16_tokens_only = True
        try:
            yield
        finally:
            neck.f16_tokens_only = before

    @staticmethod
    def _lean_head(captured):
        """The head's `lean` argument for a frame: only a captured frame drops the outputs its records do not read."""
        return bool(captured and routes.R.lean_refine2d)

    SUPPORTS_PAUSE = True
    SUPPORTS_RESTART = True

    def _activity(self, active, cold):
        """step / launch's `active` -> None (every stream takes part: today's path) or a tuple of bs bools with a False."""
        if active is None:
            return None
        mask = tuple(bool(a) for a in active)
        if len(mask) != self.bs:
            raise ValueError(f"active has {len(mask)} entries for {self.bs} streams")
        if all(mask):
            return None
        if not self.SUPPORTS_PAUSE:
            raise NotImplementedError(f"{type(self).__name__} is the single-stream form: a paused stream is a step not taken")
        if not any(mask):
            raise ValueError("no stream is active: a frame nobody takes part in is a step not taken")
        if not self.independent:
            raise ValueError("pausing a stream needs independent_streams=True (the reference's batch pads the camera groups "
                             "to the max over the batch: its streams are not independent)")
        if cold:
            raise ValueError("every stream takes part in the cold frame (a batch-wide dataflow without history)")
        return mask

    def _camera_mask(self, cameras, mask):
        """step / launch's `cameras` -> None or bs tuples of num_cams bools (normalise_cameras); the first frame with a
        missing camera switches the runner to graphs that read the staged mask (all ones = the full rig from then on)."""
        cams = normalise_cameras(cameras, self.bs, self.head.num_cams, mask)
        if cams is not None and not self.cam_masked:
            torch.cuda.synchronize(self.device)   # nothing in flight replays a graph that does not read the mask
            self._drop_graphs()
            self.cam_masked = True
        return cams

    def _carry(self, prev, metas, mask):
        """This frame's metas with the paused streams' entries held at their last active frame (whose projection matrices
        are what the host buffer of the inputs last filled still holds); the first paused frame also switches the runner to
        masked graphs."""
        if not self.masked:
            torch.cuda.synchronize(self.device)   # nothing in flight replays a graph that does not read the mask
            self._drop_graphs()
            self.masked = True
        return carry_inactive_metas(dict(img_metas=prev["img_metas"], projection_mat=self.inputs.host["proj"]), metas, mask)

    def _admit(self, prev, img, metas, active, cameras, restart=None, adopt=None):
        """What step / launch open with: the frame's activity mask, camera mask, metas (paused streams carried from `prev`,
        the metas of the frame before), checked frames, restart flags, the adoptions and the dict(img_metas=...) the frame
        is staged against (None: a cold frame). Everything that can refuse a frame does so here, before anything is enqueued.

        A frame with adoptions is staged against adopt_metas(prev, adopt). In a runner that has not decoded a frame yet it
        runs as a WARM frame in which every active slot without an adoption is restarted: `prev` is then the frame's own
        metas (what restart_metas puts there anyway) with the adopted states' entries."""
        adopt = normalise_adopt(adopt, self.bs, self.head.instance_bank.record_dims(), active, restart,
                                self.independent or self.bs == 1, self.SUPPORTS_RESTART)
        first = prev is None and adopt is not None
        if first:
            prev = dict(img_metas=list(metas["img_metas"]))
        mask = self._activity(active, prev is None)
        if first:
            given = [False] * self.bs if restart is None else [bool(r) for r in restart]
            restart = [r or (i not in adopt and (mask is None or mask[i])) for i, r in enumerate(given)]
        flags = normalise_restart(restart, self.bs, mask, prev is None, self.independent or self.bs == 1, self.SUPPORTS_RESTART)
        cams = self._camera_mask(cameras, mask)
        if mask is not None:
            metas = self._carry(prev, metas, mask)
        self._check_pose(metas, mask)
        if self.raw is not None:
            img = self._check_frames(img, mask, cams)   # (raw_surfaces: the tensors stay referenced until the frame is returned)
            self._ensure_plan(metas)
        if flags is not None:
            self.stats["restart"] = self.stats.get("restart", 0) + 1
        staged = dict(img_metas=prev["img_metas"]) if prev is not None else None
        if adopt is not None:
            self.stats["adopt"] = self.stats.get("adopt", 0) + 1
            staged = adopt_metas(staged, adopt)
        for i in range(self.bs):
            self.decoded[i] = self.decoded[i] or mask is None or mask[i]
        return mask, cams, metas, img, flags, adopt, staged

    def _import(self, adopt, stream):
        """The import launches of a frame's adoptions on `stream`, in front of its decoder -> the records as they sit on this
        device (kept by the caller until the frame is through). Importing again (a re-run) changes nothing."""
        held = []
        here = self.head.instance_bank._static["cached_feature"].device
        for slot, state in adopt.items():
            rec = state.record
            with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
                if rec.device != here:
                    state.wait()
                    rec = rec.to(here)
                elif rec.is_cuda:
                    state.wait(torch.cuda.current_stream())
                self.head.instance_bank.import_stream(slot, rec, header=state.dims)
            held.append(rec)
        return held

    def _check_export(self, s):
        """export_stream's refusals, before anything is enqueued."""
        if not self.SUPPORTS_RESTART:
            raise NotImplementedError("this runner cannot export a stream: the single-frame part of the next frame is already "
                                      "in flight when an export would have to take effect (use FrameRunner or PipelinedRunner)")
        if int(s) != s or not 0 <= int(s) < self.bs:
            raise ValueError(f"export_stream: stream {s!r} of {self.bs}")
        if self.bs > 1 and not self.independent:
            raise ValueError("exporting a stream of a batch needs independent_streams=True (the reference's batch pads the "
                             "camera groups to the max over the batch: its streams are not independent)")
        if not self.decoded[int(s)]:
            raise ValueError(f"stream {s} has not decoded a frame in this runner: there is nothing to export")
        return int(s)

    def _export(self, s, metas, stream=None, into=None):
        """Enqueue the export launch of stream s on `stream` (None: the current one) -> StreamState (into: take it again
        into this state's record). metas: the img_metas list of the frame the bank rows belong to."""
        bank = self.head.instance_bank
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            rec = bank.export_stream(s, out=into._record if into is not None else None)
            ready = None
            if rec.is_cuda:
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream())
        if into is None:
            m = metas[s]
            into = StreamState(rec, bank.record_dims(), m["T_global"], m["T_global_inv"], m["timestamp"])
        into._ready = ready
        return into

    def export_stream(self, s):
        """The state of stream s behind the last step as a StreamState: its bank rows (one launch, csrc/bank.hip) and the
        pose and time stamp of its last active frame. The slot itself does not change: pause it, restart it or adopt another
        stream into it next. Refused for a stream that has not decoded a frame here, for a batch without independent_streams
        and by the split runner."""
        s = self._check_export(s)
        return self._export(s, self.prev_metas["img_metas"])

    def _fill_inputs(self, inputs, metas, prev, mask, cams, restart=None, slot=0):
        """The frame's decoder inputs into `inputs` (host side) -> the metas dict the head reads them through. With
        camera_health the camera mask it names is the verdict of feature slot `slot`, not the host's."""
        self.inputs = inputs
        inputs.fill(metas, prev, mask, cams, self.masked, self.cam_masked, restart)
        dmetas = inputs.metas(metas["img_metas"], self.wh, self.wh_host)
        if self.health is not None:
            dmetas["camera_valid"] = self.health_slots[slot]["cam_eff"]
        return dmetas

    def _stage(self, img, metas, mask=None, cams=None, restart=None, prev="last", live=None):
        """Copy this frame's inputs into the static device buffers (a few small async copies); returns the head's metas.
        prev: what the frame is staged against (None: a cold frame); by default the metas of the frame last returned.
        live: the frame's live-image table (_idle) or None."""
        if prev == "last":
            prev = self.prev_metas
        if self.raw is None:
            self.img.copy_(img, non_blocking=True)
        else:
            self._stage_frames(self.raw, img, self.pin_table)
        self._stage_live(0, live)
        self._stage_health(0, mask, cams)
        dmetas = self._fill_inputs(self.inputs, metas, prev, mask, cams, restart)
        self.inputs.upload(torch.cuda.current_stream())
        return dmetas

    def _results(self, rec3d, rec2d, mask, world=None, count=None, health=None):
        results = self._results_of(rec3d, rec2d, mask, world, count)
        return results if health is None else self._health_results(results, health)

    def _results_of(self, rec3d, rec2d, mask, world=None, count=None):
        self.last_active = mask if mask is not None else (True,) * self.bs
        rec3d, rec2d = rec3d.numpy(), rec2d.numpy()
        if mask is None:
            results = SparseBox3DDecoder.decode_static_host(rec3d, rec2d, self.head.num_cams, self.independent)
            return self._add_world([{"img_bbox": r} for r in results], world, count)
        # independent streams: each record is a batch of one; a paused stream's rows are unspecified and are not decoded
        one = lambda i: SparseBox3DDecoder.decode_static_host(rec3d[i:i + 1], rec2d[i:i + 1], self.head.num_cams)[0]  # noqa: E731
        return self._add_world([{"img_bbox": one(i)} if a else None for i, a in enumerate(mask)], world, count)

    @staticmethod
    def _add_world(results, world, count):
        """world_output: each active stream's kept rows (views of one host copy of the frame's world record) and their number."""
        if world is None:
            return results
        world, count = world.numpy().copy(), count.numpy()
        for i, res in enumerate(results):
            if res is not None:
                n = int(count[i])
                res["img_bbox"]["world"] = dict(record=world[i, :n], count=n)
        return results

    def _frame(self, dmetas, aug_config, captured=False):
        """The device part of one frame; every tensor it returns has a fixed shape. captured: inside a graph capture."""
        feature_maps = self._extract(self.img, self.raw)
        return self._records(self.head(feature_maps, dmetas, lean=self._lean_head(captured)), aug_config, self.inputs)

    # ------------------------------------------------------------------ capacity overflow
    def _drop_graphs(self):
        self.graph = self.outputs = self.restart_graph = self.restart_outputs = None

    def _drop_all_graphs(self):
        self._drop_graphs()

    def _grow(self):
        """A frame's 2D query set did not fit: next capacity (x1.5, multiple of 128, at most anchors x cameras, which
        no set can exceed), graphs dropped. The bank still holds the state the frame found (see module docstring)."""
        bank = self.head.instance_bank
        limit = -(-bank.num_anchor * self.head.num_cams // 128) * 128
        if not bank._fusable(bank._static["cached_anchor"]) or self.capacity >= limit:
            raise RuntimeError(
                f"2D query set exceeded the static capacity {self.capacity} and the frame cannot be re-run "
                "(the instance bank is not on its fused path, so this frame's state is already committed)")
        self.capacity = min(limit, -(-max(self.capacity + 128, self.capacity * 3 // 2) // 128) * 128)
        self.head.static_capacity = self.capacity
        self.stats["overflow"] += 1
        self._drop_graphs()

    def _read_back(self, rec3d, rec2d, flags, world=None, count=None):
        if self.host3d is None or self.host2d.shape != rec2d.shape:
            self.host3d = torch.empty(rec3d.shape, dtype=rec3d.dtype).pin_memory()
            self.host2d = torch.empty(rec2d.shape, dtype=rec2d.dtype).pin_memory()
            self.host_flag = torch.empty(flags.shape, dtype=flags.dtype).pin_memory()
        if world is not None:
            if self.host_world is None:
                self.host_world = torch.empty(world.shape, dtype=world.dtype).pin_memory()
                self.host_count = torch.empty(count.shape, dtype=count.dtype).pin_memory()
            self.host_world.copy_(world, non_blocking=True)
            self.host_count.copy_(count, non_blocking=True)
        self.host3d.copy_(rec3d, non_blocking=True)
        self.host2d.copy_(rec2d, non_blocking=True)
        self.host_flag.copy_(flags, non_blocking=True)
        if self.health is not None:
            self.health_slots[0]["host"].copy_(self.health_slots[0]["flags"], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self.host3d, self.host2d, bool(self.host_flag.any())

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def step(self, img, metas, force_eager=False, active=None, cameras=None, restart=None, adopt=None):
        """One frame for all streams: img f32 [bs, cams, 3, H, W] (device; u8 [bs, cams, Hs, Ws, 3] with raw_input, u8
        [bs, cams, Hs * 3 / 2, Ws] with raw_format "nv12" / "nv21"), metas as the reference's
        test pipeline collects them (projection_mat, timestamp, img_metas with T_global/T_global_inv/
        aug_config). Returns the reference's list of {'img_bbox': {...}} (simpb_head.py:1089-1123).

        active (independent_streams only): one bool per stream; a stream with False has no frame this step. Its bank, its
        confidences and its track ids stay as they are, its rows of `img` and `metas` are ignored (they may hold anything),
        its place in the returned list holds None, and when it resumes its time step and ego-motion are measured from its
        own last frame. None or all True: every stream takes part.

        cameras: None, or one sequence of num_cams bools per stream; a camera with False delivered no frame. The stream is
        then decoded exactly as the reference decodes it when given the remaining cameras only: the camera's image slot (u8:
        anything; f32: anything finite -- the backbone still runs on it unless idle_images="skip") and its projection_mat row are ignored, its 2D
        list is empty, and bank, track ids, ego-motion and time step go on as ever: a camera that comes back simply takes
        part again. A cold frame may have missing cameras. A stream that takes part needs at least one camera (ValueError:
        pause it instead); a paused stream's row is not looked at. An overflowed frame is re-run with its own mask.

        restart: None, or one bool per stream; a stream with True begins anew in this frame -- another vehicle takes the
        slot. It is decoded exactly as a fresh runner decodes its first frame (no cached instances in the temporal attention,
        no merge, no confidence decay, track ids -1 before the frame assigns fresh ones from the batch's running counter,
        the default time step), nothing the slot held before -- bank rows, the previous pose and time stamp, NaN included --
        reaches this frame's outputs or the state it leaves, and the following frames are warm against this one. Every other
        stream is decoded as if nothing had happened (only the values of its fresh ids move with the ids the restarted
        stream takes). A batch needs independent_streams=True; a stream cannot be paused and restarted in one step, but is
        restarted in the step it resumes; on the runner's first frame the flags are ignored (everything is cold); all True
        restarts the whole batch. Frames with a True replay a graph set of their own, captured at the first such frame
        (stats["restart"] counts them); None or all False is the ordinary frame and stages nothing new.

        adopt: None, or {slot: StreamState}; the slot takes over a stream that ran elsewhere (export_stream of any runner of
        the same model) and decodes this frame WARM against that stream's own history: its record is written into the slot's
        bank rows by one launch in front of the frame (the batch's id counter is raised above every id the record carries),
        and its time step and ego-motion are measured from the state's own last frame (adopt_metas). Nothing of the slot's
        previous occupant is read. The slot must take part in the frame and cannot be restarted in it. In a runner that has
        not decoded a frame yet, the frame runs warm with every other active slot restarted. No graph changes or is captured
        anew because of an adoption (stats["adopt"] counts the frames that had one)."""
        mask, cams, metas, img, flags, adopt, prev = self._admit(self.prev_metas, img, metas, active, cameras, restart, adopt)
        aug = self._aug(metas)
        dmetas = self._stage(img, metas, mask, cams, flags, prev, self._idle(mask, cams))
        warm = prev is not None
        if adopt is not None:   # eager launches between replays, in front of the frame: no graph knows of them
            self._import(adopt, None)
        graph, outputs = (self.graph, self.outputs) if flags is None else (self.restart_graph, self.restart_outputs)
        if warm and self.use_graph and not force_eager and graph is None and self.warm_frames >= 1:
            torch.cuda.synchronize()
            if flags is not None:
                self.head.prepare_restart()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE), self._capturing():
                outputs = self._frame(dmetas, aug, captured=True)
            if flags is None:
                self.graph, self.outputs = graph, outputs
            else:
                self.restart_graph, self.restart_outputs = graph, outputs
        if warm and graph is not None and not force_eager:
            if self.rec_consumed is not None:
                torch.cuda.current_stream().wait_event(self.rec_consumed)
            graph.replay()
            rec = outputs
            self.stats["replay"] += 1
        else:
            rec = self._frame(dmetas, aug)
            self.stats["eager"] += 1
        if warm:
            self.warm_frames += 1
        rec3d, rec2d, overflow = self._read_back(*rec)
        while overflow:  # re-run the frame on the untouched bank state with a larger 2D slot array
            self._grow()
            if not warm:
                self.head.instance_bank.reset()  # a cold frame starts from an empty bank again
            self.health_hold = True   # (camera_health: the frame's verdict stands and its state has advanced)
            try:
                rec = self._frame(dmetas, aug)
            finally:
                self.health_hold = False
            self.stats["eager"] += 1
            rec3d, rec2d, overflow = self._read_back(*rec)
        self.last_rec3d, self.last_rec2d = rec[0], rec[1]
        self.prev_metas = dict(img_metas=metas["img_metas"])
        self.head.instance_bank.metas = self.prev_metas
        health = self.health_slots[0]["host"] if self.health is not None else None
        if self.world_output is None:
            return self._results(rec3d, rec2d, mask, health=health)
        self.last_world, self.last_world_count = rec[3], rec[4]
        return self._results(rec3d, rec2d, mask, self.host_world, self.host_count, health=health)


@dataclass
class Job:
    """A decoder in flight. It keeps what a re-run (_finish) stages again: the frame's metas, the metas of the frame before
    (None: a cold frame) and the frame's own activity and camera masks and restart flags."""
    slot: int
    metas: dict
    prev: dict
    rec: tuple          # the frame's device records (_records)
    done: object        # event: the records have reached the slot's pinned read-back buffers
    active: tuple
    cameras: tuple
    surfaces: list      # raw_surfaces: the frame's tensors, held until its results have been returned
    restart: tuple = None
    adopt: dict = None      # {slot: StreamState} imported in front of this frame (a re-run imports them again)
    records: list = None    # ... and their records as they sit on this device, held until the frame is through
    exports: list = None    # [(stream, StreamState)] taken behind this frame: sealed when its results are returned


class PipelinedRunner(FrameRunner):
    """FrameRunner with the backbone of frame t+1 overlapped with the decoder of frame t.

    The decoder of frame t needs the bank the decoder of frame t-1 wrote, so decoders cannot overlap
    each other; but backbone+FPN of the next frame depends on nothing but its images. Many decoder
    kernels are small and leave most of the 256 CUs idle, while the convolutions fill the chip, so the
    two run side by side on separate HIP streams: step(t) launches backbone(t) and returns the detections of
    frame t-1 (one frame of latency for throughput; flush() returns the last frame). Two feature buffers
    alternate; each (backbone, decoder) x (buffer) pair is its own hipGraph once warm, so the steady state is two
    graph launches per step.

    The decoder of frame t is ENQUEUED in step(t) as well, behind backbone(t) (an event) and behind decoder(t-1)
    (stream order): when step(t) returns with the detections of t-1, the decoder stream already holds its next
    job, and the ~0.25 ms of host work between two steps (record finish, metadata staging, graph launches) no
    longer idles it. That decoder runs before the host has seen decoder(t-1)'s overflow flags, so the bank commit
    is chained on the device: a frame's commit also holds back when the flags of the frame enqueued before it are
    set (`overflow_chain`, plugin/head.py), and collect() then re-runs both, in order, on the state frame t-1 found."""

    # the decoder of frame t is the critical path (a chain of ~170 dependent small launches); the
    # backbone of frame t+1 only has to be done by the time that chain ends: decoder stream first
    STREAM_PRIORITIES = (0, -1)             # (backbone, decoder)
    FEATURE_SLOTS = 2                       # backbone(t+1) runs beside decoder(t): a live-image table per slot, as the images

    def __init__(self, *args, **kwargs):
        """Arguments: FrameRunner's."""
        # two streams side by side from here on: a convolution that misses the in-tree kernels' shape rules must not slip to a
        # vendor kernel silently (plugin/detector.py: STRICT_NO_VENDOR)
        from .plugin import detector
        detector.STRICT_NO_VENDOR = True
        super().__init__(*args, **kwargs)
        dev = self.device
        self.s_bb = torch.cuda.Stream(device=dev, priority=self.STREAM_PRIORITIES[0])
        self.s_head = torch.cuda.Stream(device=dev, priority=self.STREAM_PRIORITIES[1])
        self.s_rec = self.s_head            # the stream the detection records are written on (for their consumers)
        if not self.SLOT_INPUTS:            # both feature slots stage through the one set: the decoders run in stream order
            self.slot_inputs = self.slot_inputs * 2
        # one input buffer per feature slot: fp32 images, or raw u8 frames (raw_input: the ingest is the first node of the
        # captured backbone graph and reads the slot's own buffer)
        self.imgs = [self.img, torch.zeros_like(self.img)] if self.raw is None else [None, None]
        self.raws = [self.raw, torch.zeros_like(self.raw)] if self.raw is not None else [None, None]
        if self.surfaces:   # one pinned address table per feature slot, reused once its copy has run (as the FrameInputs)
            self.pin_tables = [self.pin_table, torch.zeros_like(self.pin_table).pin_memory()]
            self.table_staged = [None, None]
        self.fm = [None, None]              # feature maps of the frame last produced into each slot
        self.bb_graph = [None, None]
        self.bb_out = [None, None]
        self.bb_runs = [0, 0]
        self.head_graph = [None, None]
        self.head_out = [None, None]
        self.head_runs = [0, 0]
        self.restart_graph = [None, None]   # per slot: the decoder graph of a frame that restarts a stream (FrameRunner.step)
        self.restart_out = [None, None]
        self.count = 0
        n_alloc = sum(op == "allocation" for op in self.head.operation_order)
        self.flags = torch.zeros(2, n_alloc, dtype=torch.int32, device=dev)   # overflow flags, one row per feature slot
        self.queue = []                     # decoders in flight, oldest first: Job
        self.last_metas = None              # metas of the frame whose decoder was enqueued last
        self.bb_done = [torch.cuda.Event(), torch.cuda.Event()]
        self.host = [None, None]            # pinned read-back buffers per slot: (rec3d, rec2d, flags)

    def _run_backbone(self, slot, force_eager):
        """Enqueue backbone+FPN of the image in slot `slot` on s_bb."""
        with torch.cuda.stream(self.s_bb):
            if self.use_graph and not force_eager and self.bb_graph[slot] is None and self.bb_runs[slot] >= 1:
                self.s_bb.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.s_bb, capture_error_mode=CAPTURE_MODE), self._capturing():
                    self.bb_out[slot] = self._features(slot)
                self.bb_graph[slot] = g
                self.head_graph[slot] = self.restart_graph[slot] = None  # a decoder graph bound to the old buffer is stale
                self.head_runs[slot] = 0
            if self.bb_graph[slot] is not None and not force_eager:
                self.bb_graph[slot].replay()
                self.fm[slot] = self.bb_out[slot]
            else:
                self.fm[slot] = self._features(slot)
            self.bb_runs[slot] += 1

    def _features(self, slot):
        """Backbone + FPN + token format, plus everything of the decoder that depends on the features
        alone: the value projections of the three 2D cross-attention layers."""
        fm = list(self._extract(self.imgs[slot], self.raws[slot], slot))
        if hasattr(self.head, "precompute_values") and len(fm) == 3:
            fm.append(self.head.precompute_values(fm))
        return fm

    def _decode(self, slot, dmetas, aug, inputs, captured=False):
        return self._records(self.head(self.fm[slot], dmetas, lean=self._lean_head(captured)), aug, inputs)

    def _in_flight(self):
        return len(self.queue)

    def _drop_graphs(self):
        self.head_graph, self.head_out, self.head_runs = [None, None], [None, None], [0, 0]
        self.restart_graph, self.restart_out = [None, None], [None, None]

    def _drop_all_graphs(self):
        self._drop_graphs()
        self.bb_graph, self.bb_out, self.bb_runs = [None, None], [None, None], [0, 0]

    def _new_raw_buffers(self):
        super()._new_raw_buffers()
        self.raws = [self.raw, torch.zeros_like(self.raw)]

    def _run_head(self, slot, inputs, dmetas, aug, warm, force_eager):
        """Upload the filled `inputs` and enqueue the decoder of the frame whose features sit in slot `slot`, on s_head."""
        dmetas["overflow_chain"] = (self.flags, slot)
        inputs.upload(self.s_head)
        with torch.cuda.stream(self.s_head):
            graph_ok = (self.use_graph and not force_eager and warm and self.bb_graph[slot] is not None
                        and self.fm[slot] is self.bb_out[slot])
            # a frame that restarts a stream has a graph of its own per slot, captured at the first such frame of the slot
            graphs, outs = (self.restart_graph, self.restart_out) if "restart" in dmetas else (self.head_graph, self.head_out)
            if graph_ok and graphs[slot] is None and self.head_runs[slot] >= 1:
                self.s_head.synchronize()
                if "restart" in dmetas:
                    self.head.prepare_restart()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.s_head, capture_error_mode=CAPTURE_MODE):
                    outs[slot] = self._decode(slot, dmetas, aug, inputs, captured=True)
                graphs[slot] = g
            if graph_ok and graphs[slot] is not None:
                if self.rec_consumed is not None:  # the record buffer of this graph may still be read by its consumer
                    self.s_head.wait_event(self.rec_consumed)
                graphs[slot].replay()
                rec = outs[slot]
                self.stats["replay"] += 1
            else:
                rec = self._decode(slot, dmetas, aug, inputs)
                self.stats["eager"] += 1
                if graph_ok:
                    self.head_runs[slot] += 1
            return rec

    def _enqueue_readback(self, slot, rec):
        with torch.cuda.stream(self.s_head):
            h = self.host[slot]
            if h is None or h[1].shape != rec[1].shape:
                h = tuple(torch.empty(r.shape, dtype=r.dtype).pin_memory() for r in rec)
                self.host[slot] = h
            for dst, src in zip(h, rec):
                dst.copy_(src, non_blocking=True)
            if self.health is not None:   # (written on the backbone stream in front of bb_done, which this stream waited for)
                self.health_slots[slot]["host"].copy_(self.health_slots[slot]["flags"], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.s_head)
        return done

    def _enqueue_decoder(self, slot, metas, prev, force_eager, mask=None, cams=None, surfaces=None, restart=None, adopt=None):
        """Stage the inputs of the frame whose features sit in `slot` and enqueue its decoder + read-back (_run_head); a
        frame's adoptions are imported on the decoder stream right in front of it."""
        self.prev_metas = prev   # (what the base class's helpers look at)
        inputs = self.slot_inputs[slot]
        dmetas = self._fill_inputs(inputs, metas, prev, mask, cams, restart, slot)
        records = self._import(adopt, self.s_head) if adopt is not None else None
        rec = self._run_head(slot, inputs, dmetas, self._aug(metas), prev is not None, force_eager)
        return Job(slot, metas, prev, rec, self._enqueue_readback(slot, rec), mask, cams, surfaces, restart, adopt, records)

    def export_stream(self, s):
        """FrameRunner.export_stream behind the frame launched last: the export launch is enqueued on the decoder stream
        behind that frame's decoder, with no host wait, and the state is SEALED when that frame's results are returned
        (collect, step or flush) -- the lifetime rule of raw_surfaces; using it earlier raises RuntimeError. If the frame
        (or the one in front of it) overflowed, its bank commit was held back: the export is taken again behind its re-run,
        into the same record. With nothing in flight the state is sealed at once."""
        s = self._check_export(s)
        state = self._export(s, self.last_metas["img_metas"], self.s_head)
        if self.queue:
            job = self.queue[-1]
            job.exports = (job.exports or []) + [(s, state)]
            state._sealed = False
        return state

    @torch.no_grad()
    def launch(self, img, metas, force_eager=False, active=None, cameras=None, restart=None, adopt=None):
        """Enqueue backbone(t) and decoder(t) without waiting for either (several runners -- several independent
        camera streams on one GPU -- can be launched back to back and collected after). img, active, cameras, restart, adopt:
        as FrameRunner.step (an overflowed frame, and the one enqueued behind it, are re-run each with its own flags and
        adoptions). A launch with an adoption waits for the decoder still in flight, behind enqueuing its own backbone: the
        slot's previous occupant must have committed its last frame before the adopted rows replace its own."""
        mask, cams, metas, img, flags, adopt, prev = self._admit(self.last_metas, img, metas, active, cameras, restart, adopt)
        live = self._idle(mask, cams)
        slot = self.count % 2
        cur = torch.cuda.current_stream()
        self.s_bb.wait_stream(cur)
        self.s_head.wait_stream(cur)
        with torch.cuda.stream(self.s_bb):
            self._stage_live(slot, live)   # (with the slot's images, not with the decoder's inputs: the decoder of the frame before still runs)
            self._stage_health(slot, mask, cams)
            if self.raw is None:
                self.imgs[slot].copy_(img, non_blocking=True)
            elif not self.surfaces:
                self._stage_frames(self.raws[slot], img)
            else:   # 8 * bs * cams bytes in front of the backbone graph, whose ingest node reads the slot's table
                if self.table_staged[slot] is not None:
                    self.table_staged[slot].synchronize()   # the slot's last copy out of its pinned table (long done)
                self._stage_frames(self.raws[slot], img, self.pin_tables[slot])
                self.table_staged[slot] = torch.cuda.Event()
                self.table_staged[slot].record(self.s_bb)
        self._run_backbone(slot, force_eager)
        self.bb_done[slot].record(self.s_bb)
        self.s_head.wait_event(self.bb_done[slot])
        if adopt is not None and self.queue:
            # the import replaces the slot's rows for good: the frame in flight has to have committed first -- were it to
            # overflow, its re-run would decode the slot's previous occupant against the adopted rows. The one host wait an
            # adoption costs (the backbone of this frame is enqueued already); frames without one never come here
            settled = []
            while self.queue:
                settled.append(self._settle(self.queue.pop(0)))
            self.queue.extend(settled)
        self.queue.append(self._enqueue_decoder(slot, metas, prev, force_eager, mask, cams, img[1] if self.surfaces else None,
                                                flags, adopt))
        self.last_metas = metas
        self.count += 1

    def _finish(self, job):
        """Wait for a decoder in flight, re-run it (and whatever was enqueued behind it) if its 2D set overflowed,
        return its detections."""
        job = self._settle(job)
        h = self.host[job.slot]
        for _, state in job.exports or ():
            state._sealed = True
        self.last_rec3d, self.last_rec2d = job.rec[0], job.rec[1]
        self.prev_metas = dict(img_metas=job.metas["img_metas"])
        health = self.health_slots[job.slot]["host"] if self.health is not None else None
        if self.world_output is None:
            return self._results(h[0], h[1], job.active, health=health)
        self.last_world, self.last_world_count = job.rec[3], job.rec[4]
        return self._results(h[0], h[1], job.active, h[3], h[4], health=health)

    def _settle(self, job):
        """Wait for a decoder in flight and, if its 2D set overflowed, re-run it and whatever was enqueued behind it -> the
        job whose records hold (the same one where nothing overflowed; settling it again is a no-op)."""
        job.done.synchronize()
        h = self.host[job.slot]
        if bool(h[2].any()):
            # overflow: this frame's bank commit held back, and so did the commit of the frame enqueued behind it
            # (overflow_chain); the features of both still sit in their slots -> re-run them in order, eagerly, with a
            # larger slot array (the graphs are re-captured at the new capacity afterwards)
            behind = list(self.queue)
            self.queue.clear()
            self._quiesce()
            while bool(h[2].any()):
                self._grow()
                if job.prev is None:
                    self.head.instance_bank.reset()  # a cold frame starts from an empty bank again
                self._clear_hold()   # flags left by the overflowed attempt / the speculative decoder behind it
                job = self._rerun(job)
                job.done.synchronize()
                h = self.host[job.slot]
            self.queue.extend(self._rerun(b) for b in behind)
        return job

    def _rerun(self, job):
        """The same frame again, eagerly, with its own masks and adoptions (and its surfaces still held); an export taken
        behind the first attempt found the state that attempt did not commit, and is taken again into the same record."""
        again = self._enqueue_decoder(job.slot, job.metas, job.prev, True, job.active, job.cameras, job.surfaces, job.restart,
                                      job.adopt)
        again.exports = job.exports
        for s, state in job.exports or ():
            self._export(s, job.metas["img_metas"], self.s_head, into=state)
        return again

    def _quiesce(self):
        self.s_head.synchronize()

    def _clear_hold(self):
        with torch.cuda.stream(self.s_head):
            self.flags.zero_()

    def collect(self):
        """Returns the detections of frame t-1 (None the first time): waits for the decoder enqueued one step ago,
        not for what launch() just enqueued."""
        if len(self.queue) < 2:
            return None
        return self._finish(self.queue.pop(0))

    def step(self, img, metas, force_eager=False, active=None, cameras=None, restart=None, adopt=None):
        """Feed frame t; returns the detections of frame t-1 (None on the very first call)."""
        self.launch(img, metas, force_eager, active, cameras, restart, adopt)
        return self.collect()

    @torch.no_grad()
    def flush(self):
        """Wait for the decoder of the last fed frame and return its detections."""
        out = None
        while self.queue:
            out = self._finish(self.queue.pop(0))
        return out


class SplitPipelinedRunner(PipelinedRunner):
    """PipelinedRunner with the single-frame decoder layer taken off the temporal chain.

    Frame t's decoder needs the bank frame t-1 committed -- but not from its first instruction: the first decoder layer
    (`num_single_frame_decoder`, simpb_head.py:690-696: allocation, the 2D block, aggregation, the first refinement) starts
    from the learned anchors alone, and the bank enters with InstanceBank.update behind it. SimPBHead.forward_split pauses
    there. This runner replays that first part ("A", ~1/6 of the decoder) on the backbone stream right behind backbone(t),
    beside the temporal part ("B") of frame t-1; B(t) then waits for A(t) (an event) and B(t-1) (stream order). The chain
    of dependent launches a frame adds to the critical path shrinks by A.

    What changes with A(t) running while B(t-1) is still in flight:
      * per-frame decoder inputs (projection matrices, ego-motion, time step) get one FrameInputs per feature slot;
      * the overflow hold is chained through a `sticky` word that B writes at its end (A(t+1) must not be able to disturb
        the flags B(t) looks at): SimPBHead.forward_split, `overflow_split`;
      * eager (warm-up, re-run) frames run A and B back to back on the decoder stream: only replayed graphs run A on the
        backbone stream, so no tensor of the caching allocator crosses streams.

    This is the single-stream form: it takes no paused streams (pausing its one stream means not calling step). It does
    take `cameras`: the camera mask is one more per-frame decoder input with a device buffer per feature slot. It cannot
    restart its stream (`restart=` with a True raises NotImplementedError): part A of a frame starts from the learned anchors
    and is in flight, with the time step staged for it, before the temporal part it would have to tell to start cold."""

    SUPPORTS_PAUSE = False
    SUPPORTS_RESTART = False
    SLOT_INPUTS = True

    def __init__(self, *args, **kwargs):
        """Arguments: FrameRunner's."""
        super().__init__(*args, **kwargs)
        dev = self.device
        # part A rides on the backbone stream, right behind backbone(t): as fast for one stream as a third stream of its own
        # (350 frames/s either way) and cheaper when several runners share the GPU (8 runners: 368 against 308 frames/s)
        self.s_pre = self.s_bb
        n_alloc = self.flags.shape[1]
        self.hb = torch.zeros(2, n_alloc + 1, dtype=torch.int32, device=dev)   # per slot: the frame's flags | sticky copy
        self.sticky = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pre_graph = [None, None]
        self.pre_done = [torch.cuda.Event(), torch.cuda.Event()]

    def _drop_graphs(self):
        super()._drop_graphs()
        self.pre_graph = [None, None]

    def _part_a(self, slot, dmetas, captured=False):
        gen = self.head.forward_split(self.fm[slot], dmetas, lean=self._lean_head(captured))
        next(gen)
        return gen

    def _part_b(self, gen, aug, inputs):
        try:
            gen.send(None)
        except StopIteration as done:
            outs = done.value
        else:
            raise RuntimeError("forward_split paused twice")
        return self._records(outs, aug, inputs)

    def _run_head(self, slot, inputs, dmetas, aug, warm, force_eager):
        """Upload the slot's filled `inputs` and enqueue parts A and B of the frame whose features sit in `slot`."""
        dmetas["overflow_split"] = (self.hb[slot], self.sticky)
        graph_ok = (self.use_graph and not force_eager and warm and self.bb_graph[slot] is not None
                    and self.fm[slot] is self.bb_out[slot])
        if graph_ok and self.head_graph[slot] is None and self.head_runs[slot] >= 1:
            # capture A and B of this slot (both on the decoder stream; A is replayed on the backbone stream afterwards)
            self.s_pre.synchronize()
            self.s_head.synchronize()
            inputs.upload(self.s_head)
            with torch.cuda.stream(self.s_head):
                ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(ga, stream=self.s_head, capture_error_mode=CAPTURE_MODE):
                    gen = self._part_a(slot, dmetas, captured=True)
                with torch.cuda.graph(gb, stream=self.s_head, pool=ga.pool(), capture_error_mode=CAPTURE_MODE):
                    self.head_out[slot] = self._part_b(gen, aug, inputs)
                del gen
            self.pre_graph[slot], self.head_graph[slot] = ga, gb
        if graph_ok and self.head_graph[slot] is not None:
            inputs.upload(self.s_pre)
            with torch.cuda.stream(self.s_pre):
                self.s_pre.wait_event(self.bb_done[slot])
                if self.rec_consumed is not None:   # part A shares part B's pool: the records may sit in memory A reuses
                    self.s_pre.wait_event(self.rec_consumed)
                self.pre_graph[slot].replay()
                self.pre_done[slot].record(self.s_pre)
            with torch.cuda.stream(self.s_head):
                self.s_head.wait_event(self.pre_done[slot])
                if self.rec_consumed is not None:
                    self.s_head.wait_event(self.rec_consumed)
                self.head_graph[slot].replay()
            rec = self.head_out[slot]
            self.stats["replay"] += 1
        else:
            self.s_head.wait_stream(self.s_pre)   # (covers backbone(t) and a replayed A of the other slot)
            inputs.upload(self.s_head)
            with torch.cuda.stream(self.s_head):
                rec = self._part_b(self._part_a(slot, dmetas), aug, inputs)
            self.stats["eager"] += 1
            if graph_ok:
                self.head_runs[slot] += 1
        return rec

    def _quiesce(self):
        self.s_pre.synchronize()
        self.s_head.synchronize()

    def _clear_hold(self):
        # an overflowed attempt leaves its flags and sticky = 1 (so does the speculative decoder behind it): every re-run
        # starts clean
        with torch.cuda.stream(self.s_head):
            self.sticky.zero_()
            self.hb.zero_()
