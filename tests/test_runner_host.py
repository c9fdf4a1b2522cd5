"""CPU: host-side logic of the frame runners that needs no GPU."""
import numpy as np
import torch


def test_refinement_time_step_follows_the_bank_rule():
    """runner.refinement_time_step (what SplitPipelinedRunner stages for the single-frame decoder layer, which runs before
    InstanceBank.get of its frame) against the oracle's statement of instance_bank.py:87,108-113: dt where it is non-zero
    and within max_time_interval, the default time step otherwise; f32 throughout."""
    from simpb_amd.runner import refinement_time_step
    max_dt, default = 2.0, 0.5
    dt = np.array([0.5, 0.0, 2.0, 2.0000002, -0.5, -2.5, 1e-30, 7.25, np.float32(1.9999999)], np.float32)
    got = refinement_time_step(dt, max_dt, default)
    t = torch.from_numpy(dt)
    mask = t.abs() <= max_dt                                                        # oracle/simpb_ref.py InstanceBank.get
    want = torch.where((t != 0) & mask, t, t.new_tensor(default)).numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert got[1] == np.float32(default) and got[3] == np.float32(default) and got[4] == np.float32(-0.5)


WH, BS, CAMS = (352, 128), 2, 6
MAX_DT, DEFAULT_DT = 2.0, 0.5


def _pose(b, f):
    """Pose entries (results.POSE_KEYS) of stream b at frame f: any distinct numbers will do."""
    base = 10.0 * b + f
    return dict(lidar2ego_rotation=[1.0, 0.0, 0.0, base], lidar2ego_translation=[base, 1.0, 2.0],
                ego2global_rotation=[0.5, base, 0.5, 0.5], ego2global_translation=[3.0, base, 4.0])


def _metas(f, pose_streams=(0, 1)):
    from simpb_amd import synth
    metas = synth.frame_metas(BS, f, WH, jump=(1, 2, 3.0))   # stream 1 jumps by 3 s at frame 2: a gap of 3.5 s > MAX_DT
    for b in pose_streams:
        metas["img_metas"][b].update(_pose(b, f))
    return metas


def _bits(a):
    return np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a).tobytes()


def test_frame_inputs_fill_writes_every_host_buffer():
    """FrameInputs.fill over a cold frame, a warm frame, a frame with a time jump and a frame with one paused stream carried
    through carry_inactive_metas: motion and dt are stream_motion's bit for bit, the time step is refinement_time_step's (the
    default on the cold frame), the projection is the staged one, the masks are ones or the given rows, and a stream
    without pose keys keeps its pose row."""
    from simpb_amd.results import pose_row
    from simpb_amd.runner import FrameInputs, carry_inactive_metas, refinement_time_step, stream_motion
    inp = FrameInputs(BS, CAMS, "cpu", time_step=(MAX_DT, DEFAULT_DT), pose=True)
    assert set(inp.host) == set(inp.dev) == {"proj", "t", "dt", "ti", "active", "cam", "pose"}
    for name, shape, dtype in (("proj", (BS, CAMS, 4, 4), torch.float32), ("t", (BS, 4, 4), torch.float32), ("dt", (BS,), torch.float32),
                               ("ti", (BS,), torch.float32), ("active", (BS,), torch.uint8), ("cam", (BS, CAMS), torch.uint8),
                               ("pose", (BS, 14), torch.float64)):
        for buf in (inp.host[name], inp.dev[name]):
            assert tuple(buf.shape) == shape and buf.dtype == dtype, name
    assert bool(inp.host["active"].all()) and bool(inp.host["cam"].all()) and bool(inp.dev["active"].all()) and bool(inp.dev["cam"].all())
    ones = (np.ones(BS, np.uint8), np.ones((BS, CAMS), np.uint8))

    def check(metas, prev, mask, cams, pose_rows):
        inp.fill(metas, prev, mask, cams)
        h = inp.host
        assert torch.equal(h["proj"], metas["projection_mat"].to(torch.float32))
        if prev is not None:
            t, dt = stream_motion(metas, prev)
            assert _bits(h["t"]) == _bits(t) and _bits(h["dt"]) == _bits(dt)
            assert _bits(h["ti"]) == _bits(refinement_time_step(dt, MAX_DT, DEFAULT_DT))
        else:
            assert _bits(h["ti"]) == _bits(np.full(BS, DEFAULT_DT, np.float32))
        assert np.array_equal(h["active"].numpy(), ones[0] if mask is None else np.array(mask, np.uint8))
        assert np.array_equal(h["cam"].numpy(), ones[1] if cams is None else np.array(cams, np.uint8))
        assert _bits(h["pose"]) == _bits(np.stack(pose_rows))

    m0 = _metas(0)
    check(m0, None, None, None, [pose_row(m) for m in m0["img_metas"]])                    # cold
    assert not inp.host["t"].any() and not inp.host["dt"].any()                            # (motion rows are a warm frame's)
    m1 = _metas(1, pose_streams=(0,))                                                       # warm; stream 1 brings no pose
    check(m1, m0, None, None, [pose_row(m1["img_metas"][0]), pose_row(m0["img_metas"][1])])
    assert inp.host["ti"].tolist() == [0.5, 0.5] and inp.host["dt"].tolist() == [0.5, 0.5]
    m2 = _metas(2)                                                                          # stream 1 jumps in time
    check(m2, m1, None, None, [pose_row(m) for m in m2["img_metas"]])
    assert inp.host["dt"].tolist() == [0.5, 3.5] and inp.host["ti"].tolist() == [0.5, DEFAULT_DT]
    mask, cams = (False, True), ((True,) * CAMS, (True, False, True, True, False, True))    # stream 0 sits frame 3 out
    staged = dict(img_metas=m2["img_metas"], projection_mat=inp.host["proj"])
    m3 = carry_inactive_metas(staged, _metas(3), mask)
    check(m3, m2, mask, cams, [pose_row(m2["img_metas"][0]), pose_row(m3["img_metas"][1])])
    assert inp.host["dt"].tolist() == [0.0, 0.5] and inp.host["ti"].tolist() == [DEFAULT_DT, 0.5]
    assert torch.equal(inp.host["proj"][0], m2["projection_mat"][0].to(torch.float32))
    m4 = _metas(4)                                                                          # everyone back: the masks are ones again
    check(m4, m3, None, None, [pose_row(m) for m in m4["img_metas"]])
    assert inp.host["dt"].tolist() == [1.0, 0.5]                                            # stream 0 measures from its own last frame

    bare = FrameInputs(BS, CAMS, "cpu")
    assert set(bare.host) == set(bare.dev) == {"proj", "t", "dt", "active", "cam"}
    bare.fill(m1, m0, None, None)
    assert _bits(bare.host["t"]) == _bits(stream_motion(m1, m0)[0])


def test_frame_inputs_metas_has_the_key_sets_of_the_three_runners():
    """FrameInputs.metas: the head's dict over the device buffers. Cold: the four plain keys; warm: bank_inputs too; `active`
    and `camera_valid` only for a runner whose graphs read the masks; `time_interval` only where the time-step buffer
    exists (the split runner's sets). wh is passed in at every call (the runner's attributes, which may be re-assigned)."""
    from simpb_amd.runner import FrameInputs
    m0, m1 = _metas(0), _metas(1)
    wh, wh_host = torch.tensor([float(WH[0]), float(WH[1])]).view(1, 1, 2).repeat(BS, CAMS, 1), WH
    plain = {"projection_mat", "image_wh", "image_wh_host", "img_metas"}
    for time_step, extra in ((None, set()), ((MAX_DT, DEFAULT_DT), {"time_interval"})):
        inp = FrameInputs(BS, CAMS, "cpu", time_step=time_step)
        d = inp.dev
        inp.fill(m0, None, None, None)
        assert set(inp.metas(m0["img_metas"], wh, wh_host)) == plain | extra
        inp.fill(m1, m0, None, None)
        out = inp.metas(m1["img_metas"], wh, wh_host)
        assert set(out) == plain | extra | {"bank_inputs"}
        assert out["projection_mat"] is d["proj"] and out["bank_inputs"][0] is d["t"] and out["bank_inputs"][1] is d["dt"]
        assert out["image_wh"] is wh and out["image_wh_host"] is wh_host and out["img_metas"] is m1["img_metas"]
        assert ("time_interval" in out) == (time_step is not None) and out.get("time_interval") is d.get("ti")
        inp.fill(m1, m0, None, None, masked=True)
        out = inp.metas(m1["img_metas"], wh, wh_host)
        assert set(out) == plain | extra | {"bank_inputs", "active"} and out["active"] is d["active"]
        inp.fill(m1, m0, None, None, cam_masked=True)
        out = inp.metas(m1["img_metas"], wh, wh_host)
        assert set(out) == plain | extra | {"bank_inputs", "camera_valid"} and out["camera_valid"] is d["cam"]
        inp.fill(m0, None, None, None, masked=True, cam_masked=True)
        assert set(inp.metas(m0["img_metas"], wh, wh_host)) == plain | extra | {"active", "camera_valid"}
