"""CPU: the host side of per-stream pause / resume (runner.carry_inactive_metas + runner.stream_motion, the two pure
functions FrameRunner / PipelinedRunner stage a frame with) and the argument validation of the three `_active` entry
points, which runs before any HIP call."""
import ctypes

import numpy as np
import torch

from simpb_amd import _lib, build, synth
from simpb_amd.runner import carry_inactive_metas, stream_motion

WH = (352, 128)


def _walk(schedule, bs=2, other_rig=None):
    """Drive the two functions the way the runners do: frame 0 is cold (everyone active), every later frame is carried
    against the previous frame's staged metas when its mask has a False, staged against them, and becomes `prev`. Returns per
    step (metas as given, metas as staged, T, dt)."""
    prev, out = None, []
    for step, mask in enumerate(schedule):
        metas = synth.frame_metas(bs, step, WH)
        if other_rig is not None:   # what an inactive stream's row holds must not matter
            for i, a in enumerate(mask):
                if not a:
                    metas["projection_mat"][i] = other_rig
        staged = metas if all(mask) else carry_inactive_metas(prev, metas, mask)
        t = dt = None
        if prev is not None:
            t, dt = stream_motion(staged, prev)
        out.append((metas, staged, t, dt))
        prev = dict(img_metas=staged["img_metas"], projection_mat=staged["projection_mat"])
    return out


def test_resumed_stream_measures_time_and_ego_motion_from_its_own_last_frame():
    schedule = [(True, True), (True, True), (True, False), (True, False), (True, True)]
    other = torch.full((6, 4, 4), 7.0)
    steps = _walk(schedule, other_rig=other)
    pose = lambda b, k: steps[k][0]["img_metas"][b]   # noqa: E731  (the frame as the caller delivered it)
    for k in range(1, 5):
        _, staged, t, dt = steps[k]
        assert t.dtype == np.float32 and dt.dtype == np.float32 and t.shape == (2, 4, 4) and dt.shape == (2,)
        # stream 0 never pauses: half a second and one step of ego-motion, every frame
        assert dt[0] == np.float32(0.5)
        assert np.array_equal(t[0], np.asarray(pose(0, k)["T_global_inv"] @ pose(0, k - 1)["T_global"], np.float32))
        assert staged["img_metas"][0] is steps[k][0]["img_metas"][0]
    for k in (2, 3):   # paused: its own entries are those of its last active frame (step 1), so nothing moves
        _, staged, t, dt = steps[k]
        assert staged["img_metas"][1] is steps[1][0]["img_metas"][1]
        assert torch.equal(staged["projection_mat"][1], steps[1][0]["projection_mat"][1])
        assert torch.equal(staged["projection_mat"][0], steps[k][0]["projection_mat"][0])
        assert dt[1] == 0.0
        assert np.abs(t[1] - np.eye(4, dtype=np.float32)).max() <= 1e-6
        assert steps[k][0]["projection_mat"][1, 0, 0, 0] == 7.0   # the caller's tensor is not written
    _, staged, t, dt = steps[4]
    assert dt[1] == np.float32(1.5)
    assert np.array_equal(t[1], np.asarray(pose(1, 4)["T_global_inv"] @ pose(1, 1)["T_global"], np.float32))
    assert staged["img_metas"][1] is steps[4][0]["img_metas"][1]


def test_aug_config_survives_stream_zero_sitting_out():
    prev = synth.frame_metas(2, 0, WH)
    prev["img_metas"][0]["aug_config"] = dict(resize=0.5, crop=(1, 2, 3, 4))
    metas = synth.frame_metas(2, 1, WH)
    metas["img_metas"][0] = {}   # a stream without a frame need not deliver anything
    staged = carry_inactive_metas(prev, metas, [False, True])
    assert staged["img_metas"][0]["aug_config"] == dict(resize=0.5, crop=(1, 2, 3, 4))
    assert staged["img_metas"][1] is metas["img_metas"][1]
    assert metas["img_metas"][0] == {} and "timestamp" in staged
    t, dt = stream_motion(staged, prev)
    assert dt.tolist() == [0.0, 0.5]


def test_carry_rejects_a_mask_of_the_wrong_length():
    prev, metas = synth.frame_metas(2, 0, WH), synth.frame_metas(2, 1, WH)
    try:
        carry_inactive_metas(prev, metas, [True, False, True])
    except ValueError:
        return
    raise AssertionError("a mask of three entries for two streams was accepted")


def test_active_entry_points_validate_before_any_hip_call():
    """As tests/test_capi.py::test_bad_arguments_return_einval: no device in the process."""
    build.build_extension()
    h = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)
    P = lambda n, v: [v] * n   # noqa: E731
    # simpb_alloc_ragged_active: 15 pointers, bs, A, cams, per_stream, 5 floats, active, stream
    assert h.simpb_alloc_ragged_active(*P(15, null), 3, 48, 6, 128, 704.0, 256.0, 35.0, 35.0, 10.0, one, null) == 1
    assert h.simpb_alloc_ragged_active(*P(15, null), 3, 48, 6, 128, 704.0, 256.0, 35.0, 35.0, 10.0, null, null) == 1
    assert h.simpb_alloc_ragged_active(*P(15, one), 17, 48, 6, 128, 704.0, 256.0, 35.0, 35.0, 10.0, one, null) == 1   # 102 groups
    assert h.simpb_alloc_ragged_active(*P(15, one), 3, 48, 6, 0, 704.0, 256.0, 35.0, 35.0, 10.0, one, null) == 1
    # simpb_bank_update_merge_active: 13 pointers (.., mask, hold), num_hold, sticky, bs, A, T, C, E, active, stream
    assert h.simpb_bank_update_merge_active(*P(13, null), 0, null, 3, 48, 32, 16, 0, one, null) == 1
    assert h.simpb_bank_update_merge_active(*P(13, one), 0, null, 3, 48, 48, 16, 0, one, null) == 1   # T must be < A
    assert h.simpb_bank_update_merge_active(*P(13, one), 0, null, 3, 48, 32, 18, 0, one, null) == 1   # C % 4
    # simpb_bank_cache_streams_active: 10 pointers, bs, A, classes, T, C, has_prev, decay, has_thr, thr, hold, num_hold,
    # sticky, sync, active, stream
    assert h.simpb_bank_cache_streams_active(*P(10, null), 3, 48, 10, 32, 16, 1, 0.6, 0, 0.0, null, 0, null, one, one, null) == 1
    assert h.simpb_bank_cache_streams_active(*P(10, null), 3, 48, 10, 32, 16, 1, 0.6, 0, 0.0, null, 0, null, null, one, null) == 1
    assert h.simpb_bank_cache_streams_active(*P(10, one), 3, 2000, 10, 32, 16, 1, 0.6, 0, 0.0, null, 0, null, one, one, null) == 1
    assert h.simpb_bank_cache_streams_active(*P(10, one), 3, 48, 10, 32, 16, 1, 0.6, 0, 0.0, null, 2, null, one, one, null) == 1
    assert h.simpb_abi_version() == 7
