"""CPU: the world record's host side (simpb_amd/results.py: world_tables, world_record_host, annos_from_world) against the per-box
format_sample it restates, and the argument checks of the C entry point (csrc/world.hip)."""
import ctypes
import json

import numpy as np
import pytest

from simpb_amd import _lib, results
from tests import world_cases as W


@pytest.fixture(scope="module")
def sample():
    """One random sample: info (pose + token) and a 300-box record with nothing near a cut. Never modified."""
    rng = np.random.default_rng(20240607)
    info = dict(W.random_pose(rng), token="tok-0")
    rec = W.random_record(rng, 300, info)
    ids = np.ascontiguousarray(rec[:, 13:15]).view(np.int64)[:, 0]
    assert (ids == -1).any() and (ids > 2 ** 33).any()
    assert abs(np.linalg.norm(info["ego2global_rotation"]) - 1) > 1e-3 and abs(np.linalg.norm(info["lidar2ego_rotation"]) - 1) > 1e-3
    return info, rec


@pytest.mark.parametrize("threshold", [None, W.THRESHOLD])
@pytest.mark.parametrize("tracking", [False, True])
def test_world_record_host_equals_format_sample(sample, tracking, threshold):
    info, rec = sample
    want = results.format_sample(W.det_of(rec), info, W.CLASSES, tracking, threshold)
    tables = results.world_tables(W.CLASSES, tracking)
    world, count = results.world_record_host(rec[None], results.pose_row(info)[None], tables, threshold)
    assert world.shape == (1, 300, 16) and world.dtype == np.float64 and count.dtype == np.int32
    assert 0 < count[0] == len(want) < 300   # every mode cuts something, none cuts everything
    W.assert_same_annos(results.annos_from_world(world[0], count[0], info["token"], W.CLASSES, tracking), want, tracking)
    if not tracking:   # both sides of the speed cut are present
        assert len({a["attribute_name"] for a in want if a["detection_name"] == "car"}) == 2
    pad = world[0, count[0]:]
    assert np.array_equal(pad[:, 13], np.full(len(pad), -1.0)) and not np.delete(pad, 13, axis=1).view(np.int64).any()


def test_boxes_exactly_on_a_cut():
    rec, kept = W.exact_cuts()
    info = dict(W.IDENTITY_POSE, token="tok-cut")
    want = results.format_sample(W.det_of(rec), info, W.CLASSES, False, 0.25)
    assert [a["translation"] for a in want] == [[1.0, 2.0, 0.0], [30.0, 40.0, 0.0]] and want[1]["detection_name"] == "car"
    world, count = results.world_record_host(rec[None], results.pose_row(info)[None], results.world_tables(W.CLASSES, False), 0.25)
    assert count[0] == len(kept)
    W.assert_same_annos(results.annos_from_world(world[0], count[0], "tok-cut", W.CLASSES), want, False)
    assert np.array_equal(world[0, :2, 0:3], rec[kept, 0:3].astype(np.float64))
    assert np.array_equal(np.ascontiguousarray(world[0, :2, 15]).view(np.int64), [7, 2 ** 34 + 1])


def test_inactive_stream_and_tables():
    rng = np.random.default_rng(5)
    infos = [W.random_pose(rng) for _ in range(2)]
    rec = np.stack([W.random_record(rng, 40, i) for i in infos])
    pose = np.stack([results.pose_row(i) for i in infos])
    rec[1] = np.nan   # a paused stream's rows may hold anything
    tables = results.world_tables(W.CLASSES, True)
    world, count = results.world_record_host(rec, pose, tables, None, active=[1, 0])
    assert count[1] == -1 and count[0] > 0
    assert np.array_equal(world[1, :, 13], np.full(40, -1.0)) and not np.delete(world[1], 13, axis=1).any()
    for name in results.TRACKING_DROPPED:
        assert tables["class_range"][W.CLASSES.index(name)] < 0
    assert (tables["class_range"][len(W.CLASSES):] < 0).all()
    det = results.world_tables(W.CLASSES, False)
    names = results.ATTRIBUTE_NAMES
    bus, ped = W.CLASSES.index("bus"), W.CLASSES.index("pedestrian")
    assert (names[det["attr_moving"][bus]], names[det["attr_still"][bus]]) == ("vehicle.moving", "vehicle.stopped")
    assert (names[det["attr_moving"][ped]], names[det["attr_still"][ped]]) == ("pedestrian.moving", "pedestrian.standing")
    assert det["class_range"][bus] == 50 and det["class_range"][ped] == 40
    with pytest.raises(ValueError):
        results.world_tables(["car"] * 33, False)


def test_write_submission_takes_world_records(sample, tmp_path):
    info, rec = sample
    a = results.write_submission([W.det_of(rec)], [info], W.CLASSES, str(tmp_path / "a.json"), tracking=True, threshold=W.THRESHOLD)
    world, count = results.world_record_host(rec[None], results.pose_row(info)[None], results.world_tables(W.CLASSES, True),
                                             W.THRESHOLD)
    b = results.write_submission(None, [info], W.CLASSES, str(tmp_path / "b.json"), tracking=True,
                                 world_records=[dict(record=world[0], count=int(count[0]))])
    a, b = json.load(open(a)), json.load(open(b))
    assert a["meta"] == b["meta"] and list(a["results"]) == list(b["results"]) == ["tok-0"]
    W.assert_same_annos(b["results"]["tok-0"], a["results"]["tok-0"], True)


def test_world_record_bad_arguments_return_einval():
    """As tests/test_capi.py::test_bad_arguments_return_einval: validation runs before any HIP call."""
    h = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    t = _lib.WorldTables()
    t.num_output = 513   # above the 512 rows a workgroup holds
    assert h.simpb_world_record(one, one, one, one, null, t, 1, null) == 1
    t.num_output = 300
    for args in ((null, one, one, one), (one, null, one, one), (one, one, null, one), (one, one, one, null)):
        assert h.simpb_world_record(*args, null, t, 1, null) == 1
    assert h.simpb_world_record(one, one, one, one, null, t, 0, null) == 1
    assert h.simpb_world_record(ctypes.c_void_p(72), one, one, one, null, t, 1, null) == 1   # record not 16-byte aligned
