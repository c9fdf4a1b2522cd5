"""The schedule the per-stream restart tests share (CPU and GPU): three streams of the small head of
tests/test_gpu_stream_activity.py over seven steps.

    stream 0: active at steps 0 1 2 3 4 5 6     never restarted
    stream 1: active at steps 0 1 2 R 4 5 6     restarted at step 3
    stream 2: active at steps 0 1 . . R 5 6     paused at steps 2-3, restarted at step 4, the step it resumes

A restarted slot is taken by ANOTHER VEHICLE: other tokens (the feature maps of step + 10), another camera rig, a T_global
more than a kilometre away under another yaw, and a time stamp 1 s EARLIER than the slot's last one -- within
max_time_interval, so the reference's own mask rule would keep the old history: only the restart breaks it. No GPU here."""
import functools

import numpy as np
import torch

from simpb_amd import synth

WH, BS, CAMS = (352, 128), 3, 6
STEPS = 7
ACTIVE = [(True, True, True), (True, True, True), (True, True, False), (True, True, False), (True, True, True),
          (True, True, True), (True, True, True)]
RESTART = [None, None, None, (False, True, False), (False, False, True), None, None]
RESTART_AT = {1: 3, 2: 4}          # stream -> the step it restarts at
TIME_SHIFT = {1: -1.5, 2: -2.5}    # the new vehicle's clock against the old one's: dt = -1.0 s at the restart frame


@functools.lru_cache(maxsize=None)
def maps(idx):
    """Feature maps of frame `idx` as f16 numbers (what the fp16 FPN leaves), on the host; never modified."""
    return tuple(m.half().float() for m in synth.feature_maps_nchw(BS, idx, WH))


def generation(stream, step, restarts=True):
    """0: the slot's first vehicle; 1: the vehicle that takes it at the stream's restart step."""
    return int(restarts and stream in RESTART_AT and step >= RESTART_AT[stream])


def other_rig():
    return torch.from_numpy(synth.camera_rig(WH, height=2.5, forward_offset=-1.0))


def _far(pose, stream):
    """The pose of a vehicle somewhere else: turned by a radian or two, more than a kilometre away."""
    th = 1.0 + 0.7 * stream
    turn = np.eye(4)
    turn[0, 0], turn[0, 1], turn[1, 0], turn[1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    turn[:3, 3] = (1500.0 + 400.0 * stream, -900.0, 3.0)
    return turn @ pose


def frame(step, restarts=True):
    """(maps, metas) of a step: each stream's rows are those of the vehicle that holds its slot. A paused stream's rows are
    there as well (nobody reads them)."""
    base, metas = maps(step), synth.frame_metas(BS, step, WH)
    out = [m.clone() for m in base]
    for b in range(BS):
        if not generation(b, step, restarts):
            continue
        for lvl, m in enumerate(maps(step + 10)):
            out[lvl][b] = m[b]
        metas["projection_mat"][b] = other_rig()
        t = float(metas["timestamp"][b]) + TIME_SHIFT[b]
        pose = _far(synth.ego_pose(t), b)
        metas["timestamp"][b] = t
        metas["img_metas"][b] = dict(metas["img_metas"][b], T_global=pose, T_global_inv=np.linalg.inv(pose), timestamp=t)
    return tuple(out), metas


def one_stream(metas, b):
    """Stream b of a frame's metas as a batch of one."""
    return dict(projection_mat=metas["projection_mat"][b:b + 1], image_wh=metas["image_wh"][b:b + 1],
                timestamp=metas["timestamp"][b:b + 1], img_metas=[metas["img_metas"][b]])


def pairs():
    """Every active (step, stream) of the schedule, and whether it is a restart pair."""
    return [(step, b, RESTART[step] is not None and RESTART[step][b]) for step in range(STEPS) for b in range(BS) if ACTIVE[step][b]]
