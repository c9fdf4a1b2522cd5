"""CPU: the host side of a per-stream restart (runner.normalise_restart, runner.restart_metas, FrameInputs) and the oracle's
own tie margins over the schedule the GPU tests run (tests/stream_restart_schedule.py)."""
import numpy as np
import pytest
import torch

from tests import stream_restart_schedule as S


# ------------------------------------------------------------------------------------------------------- 1. argument rules
def test_restart_flags_are_normalised_and_refused_by_the_rules():
    from simpb_amd.runner import normalise_restart
    assert normalise_restart(None, 3) is None
    assert normalise_restart([False, False, False], 3) is None and normalise_restart([0, 0, 0], 3, active=(True, False, True)) is None
    assert normalise_restart([0, 1, 0], 3) == (False, True, False)
    assert normalise_restart([1, 1, 1], 3) == (True, True, True)                       # a batch-wide restart: the same path
    assert normalise_restart(np.array([0, 1, 0]), 3, active=None) == (False, True, False)
    assert normalise_restart([True], 1, independent=True) == (True,)
    # the runner's first frame: accepted and ignored (everything is cold already) -- but a wrong length is still refused
    assert normalise_restart([0, 1, 0], 3, cold=True) is None
    for bad in ([True], [True] * 4, []):
        with pytest.raises(ValueError):
            normalise_restart(bad, 3)
        with pytest.raises(ValueError):
            normalise_restart(bad, 3, cold=True)
    with pytest.raises(ValueError):                                                     # the reference's padded batch
        normalise_restart([0, 1, 0], 3, independent=False)
    assert normalise_restart([0, 0, 0], 3, independent=False) is None
    with pytest.raises(ValueError):                                                     # paused and restarted at once
        normalise_restart([0, 1, 0], 3, active=(True, False, True))
    assert normalise_restart([0, 1, 0], 3, active=(True, True, False)) == (False, True, False)   # restarted as it resumes
    with pytest.raises(ValueError):
        normalise_restart([0, 1, 0], 3, active=(True, True))
    with pytest.raises(NotImplementedError):                                            # the split runner
        normalise_restart([True], 1, supported=False)
    with pytest.raises(NotImplementedError):
        normalise_restart([True], 1, cold=True, supported=False)
    assert normalise_restart([False], 1, supported=False) is None


def test_runner_classes_declare_what_they_support():
    from simpb_amd.runner import FrameRunner, PipelinedRunner, SplitPipelinedRunner
    assert FrameRunner.SUPPORTS_RESTART and PipelinedRunner.SUPPORTS_RESTART and not SplitPipelinedRunner.SUPPORTS_RESTART


# ------------------------------------------------------------------------------------------------------ 2. staged motion
def _nan_entry(m):
    bad = np.full((4, 4), np.nan)
    return dict(m, T_global=bad, T_global_inv=bad, timestamp=float("nan"))


def test_restart_metas_is_pure_and_never_reads_the_previous_occupant():
    from simpb_amd.runner import FrameInputs, restart_metas, stream_motion
    _, prev = S.frame(2)
    _, cur = S.frame(3)
    flags = S.RESTART[3]
    before = ([dict(m) for m in prev["img_metas"]], [dict(m) for m in cur["img_metas"]])
    staged = restart_metas(dict(img_metas=prev["img_metas"]), cur, flags)
    for old, new in zip(before, (prev["img_metas"], cur["img_metas"])):                 # nothing modified
        assert all(o.keys() == n.keys() and all(o[k] is n[k] for k in o) for o, n in zip(old, new))
    assert staged["img_metas"][1] is cur["img_metas"][1] and staged["img_metas"][0] is prev["img_metas"][0]
    t, dt = stream_motion(cur, staged)
    assert dt[1] == 0.0 and dt[0] == np.float32(0.5) and dt[2] == np.float32(0.5)
    assert np.allclose(t[1], np.eye(4), atol=1e-6) and np.isfinite(t).all()
    # the previous occupant's pose and time stamp as NaN: the staged motion is the same bytes
    poisoned = dict(img_metas=[_nan_entry(m) if f else m for f, m in zip(flags, prev["img_metas"])])
    t2, dt2 = stream_motion(cur, restart_metas(poisoned, cur, flags))
    assert t.tobytes() == t2.tobytes() and dt.tobytes() == dt2.tobytes()
    with pytest.raises(ValueError):
        restart_metas(dict(img_metas=prev["img_metas"]), cur, (True, False))

    inp = FrameInputs(S.BS, S.CAMS, "cpu", time_step=(2.0, 0.5))
    wh = torch.zeros(S.BS, S.CAMS, 2)
    inp.fill(cur, dict(img_metas=prev["img_metas"]), None, None)                        # no flags: nothing new anywhere
    assert not inp.restarting and "restart" not in inp.metas(cur["img_metas"], wh, S.WH)
    assert inp.host["dt"].tolist() == [0.5, -1.0, 0.5] and not inp.restart_host.any()
    inp.fill(cur, poisoned, None, None, restart=flags)
    out = inp.metas(cur["img_metas"], wh, S.WH)
    assert inp.restarting and out["restart"] is inp.restart_dev and inp.restart_host.tolist() == [0, 1, 0]
    assert inp.host["t"].numpy().tobytes() == t.tobytes() and inp.host["dt"].tolist() == [0.5, 0.0, 0.5]
    assert inp.host["ti"].tolist() == [0.5, 0.5, 0.5]                                   # dt = 0: the default time step
    inp.fill(cur, None, None, None, restart=flags)                                      # a cold frame ignores the flags
    assert not inp.restarting and "restart" not in inp.metas(cur["img_metas"], wh, S.WH)


def test_the_schedule_is_what_its_docstring_says():
    """Both restarts are a new vehicle by every criterion, with |dt| inside max_time_interval: only the restart can break the
    history there."""
    last = {}
    for step in range(S.STEPS):
        _, metas = S.frame(step)
        for b in range(S.BS):
            if not S.ACTIVE[step][b]:
                continue
            m = metas["img_metas"][b]
            if S.RESTART[step] is not None and S.RESTART[step][b]:
                old = last[b]
                assert -2.0 <= m["timestamp"] - old["timestamp"] < 0.0
                assert np.linalg.norm(m["T_global"][:3, 3] - old["T_global"][:3, 3]) > 1000.0
                assert abs(np.arctan2(m["T_global"][1, 0], m["T_global"][0, 0]) - np.arctan2(old["T_global"][1, 0], old["T_global"][0, 0])) > 0.5
                assert not torch.equal(metas["projection_mat"][b], S.frame(step, restarts=False)[1]["projection_mat"][b])
                assert not torch.equal(S.frame(step)[0][0][b], S.frame(step, restarts=False)[0][0][b])
                assert not S.ACTIVE[step - 1][b] or b == 1
            last[b] = m
    assert [p[:2] for p in S.pairs() if p[2]] == [(3, 1), (4, 2)] and len(S.pairs()) == 19


# ------------------------------------------------------------------------------------------------- 3. the oracle's margins
def test_oracle_margins_over_the_schedule_stay_inside_the_cap():
    """The oracle alone, one chain per vehicle (a fresh OracleHead at a restart, its prev_id carried over): the three margins
    of tests/test_gpu_stream_activity.py::_tie_evidence for every pair of the schedule. The GPU comparison excuses a miss
    only by a margin < 1e-4, for at most 2 pairs and for NO restart pair -- a condition the oracle's own numbers must leave
    room for: at most 2 pairs below 1e-4 here, and neither restart pair."""
    from oracle import simpb_ref as R
    from tests.helpers import build_product_head
    from tests.test_gpu_stream_activity import SPEC, _tie_evidence
    head = build_product_head(SPEC, device="cpu")
    params = {k: v.detach().cpu() for k, v in head.state_dict().items()}
    A, T, N = SPEC["num_anchor"], SPEC["num_temp"], SPEC["num_output"]
    torch.set_num_threads(16)
    chains, tight = [None] * S.BS, []
    with torch.no_grad():
        for step in range(S.STEPS):
            maps, metas = S.frame(step)
            fm = R.feature_maps_format(list(maps))
            for b in range(S.BS):
                if not S.ACTIVE[step][b]:
                    continue
                cold = S.RESTART[step] is not None and S.RESTART[step][b]
                if chains[b] is None or cold:
                    prev_id = chains[b].bank.prev_id if chains[b] is not None else 0
                    chains[b] = R.OracleHead(params, head.operation_order, A, T, N)
                    chains[b].bank.prev_id = prev_id
                one = S.one_stream(metas, b)
                want = chains[b].forward([fm[0][b:b + 1], fm[1], fm[2]], one)
                anchors = [chains[b].p["instance_bank.anchor"][None]] + list(want["prediction"])
                tie = _tie_evidence(want, one, T, N, anchors)
                print("oracle margins: step %d stream %d%s: %s" % (step, b, " (restart)" if cold else "", tie))
                if min(tie.values()) < 1e-4:
                    tight.append((step, b, cold, tie))
    assert len(tight) <= 2 and not any(t[2] for t in tight), tight
