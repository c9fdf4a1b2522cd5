"""Inputs shared by the world-record tests (tests/test_world_record_host.py, tests/test_gpu_world_record.py): random detection
records and poses with no box near a cut, and the hand-made boxes that sit exactly on one."""
import numpy as np

from simpb_amd import results

CLASSES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
           "traffic_cone")
THRESHOLD = 0.2
MARGIN = 1e-6   # no random box lies this close to a cut (class range, speed 0.2, threshold)
TOL = 1e-9      # float lanes: < 40 double operations on magnitudes up to 2^14 -> 40 * 2^-53 * 2^14 = 7e-11, x10 and more for
                # contraction and sincos


def random_pose(rng):
    """A sample info with raw (NOT normalised) quaternions and a global translation of up to +-8 000 m."""
    def quat(tilt):
        q = np.array([rng.normal(), tilt * rng.normal(), tilt * rng.normal(), rng.normal()])
        return q / np.linalg.norm(q) * rng.uniform(0.5, 2.0)
    return dict(lidar2ego_rotation=quat(0.05).tolist(), lidar2ego_translation=rng.uniform(-2, 2, 3).tolist(),
                ego2global_rotation=quat(0.1).tolist(),
                ego2global_translation=[rng.uniform(-8000, 8000), rng.uniform(-8000, 8000), rng.uniform(-50, 50)])


IDENTITY_POSE = dict(lidar2ego_rotation=[1.0, 0.0, 0.0, 0.0], lidar2ego_translation=[0.0, 0.0, 0.0],
                     ego2global_rotation=[1.0, 0.0, 0.0, 0.0], ego2global_translation=[0.0, 0.0, 0.0])


def set_ids(rec, ids):
    rec.view(np.uint32)[..., 13:15] = np.ascontiguousarray(ids, dtype=np.int64).view(np.uint32).reshape(ids.shape + (2,))


def _draw(rng, n, spread):
    rec = np.zeros((n, 15), np.float32)
    rec[:, 0:2] = rng.uniform(-spread, spread, (n, 2))
    rec[:, 2] = rng.uniform(-3, 3, n)
    rec[:, 3:6] = rng.uniform(0.3, 12, (n, 3))
    rec[:, 6] = rng.uniform(-np.pi, np.pi, n)
    rec[:, 7:9] = rng.normal(size=(n, 2)) * rng.choice([0.05, 3.0], (n, 1))   # speeds on both sides of 0.2
    rec[:, 9] = 0.1 * rng.normal(size=n)
    rec[:, 10] = rng.uniform(0, 1, n)
    rec[:, 11] = rng.integers(0, len(CLASSES), n)
    rec[:, 12] = rng.uniform(0, 1, n)
    ids = rng.integers(0, 2 ** 40, n)
    ids[rng.uniform(size=n) < 0.1] = -1
    ids[rng.uniform(size=n) < 0.3] += 2 ** 33
    set_ids(rec, ids)
    return rec


def cut_margins(rec, info):
    """Per box, the distance to each of the three cuts, from the quantities format_sample itself compares: the ego-frame
    distance against the class range, the global-frame speed against 0.2, the score before the re-score against THRESHOLD."""
    box = rec[:, :10].astype(np.float64)
    r1 = results.quat_rotmat(np.asarray(info["lidar2ego_rotation"], np.float64))
    r2 = results.quat_rotmat(np.asarray(info["ego2global_rotation"], np.float64))
    centre = box[:, :3] @ r1.T + np.asarray(info["lidar2ego_translation"], np.float64)
    vel = np.concatenate([box[:, 7:9], np.zeros((len(box), 1))], 1) @ r1.T @ r2.T
    rng_of = np.array([results.CLASS_RANGE[CLASSES[int(c)]] for c in rec[:, 11]], np.float64)
    return np.stack([np.abs(np.linalg.norm(centre[:, :2], axis=1) - rng_of), np.abs(np.hypot(vel[:, 0], vel[:, 1]) - 0.2),
                     np.abs(rec[:, 12].astype(np.float64) - THRESHOLD)], 1)


def random_record(rng, k, info, spread=60.0):
    """f32 [k, 15] as decode3d writes it (scores descending), ids including -1 and values above 2^33; boxes within MARGIN of a
    cut are drawn again until none is left (asserted)."""
    rec = _draw(rng, k, spread)
    for _ in range(100):
        bad = np.nonzero((cut_margins(rec, info) <= MARGIN).any(1))[0]
        if not len(bad):
            break
        rec[bad] = _draw(rng, len(bad), spread)
    rec[:, 10] = -np.sort(-rec[:, 10])
    assert (cut_margins(rec, info) > MARGIN).all()
    return rec


def exact_cuts():
    """Three boxes ON a cut, under IDENTITY_POSE and threshold 0.25: score == threshold (kept); a car at (30, 40, 0), i.e. at
    exactly 50 m (kept: the range test is `>`); a pedestrian at the same place (dropped). -> (rec f32 [3, 15], kept rows)."""
    rec = np.zeros((3, 15), np.float32)
    rec[:, 3:6] = (1.9, 4.5, 1.6)
    rec[:, 10] = (0.9, 0.8, 0.7)
    rec[0, 0:3], rec[0, 11], rec[0, 12] = (1.0, 2.0, 0.0), CLASSES.index("car"), 0.25
    rec[1, 0:3], rec[1, 11], rec[1, 12] = (30.0, 40.0, 0.0), CLASSES.index("car"), 0.5
    rec[2, 0:3], rec[2, 11], rec[2, 12] = (30.0, 40.0, 0.0), CLASSES.index("pedestrian"), 0.5
    set_ids(rec, np.array([7, 2 ** 34 + 1, 9]))
    return rec, [0, 1]


def det_of(rec):
    """One stream's record as the result dict format_sample takes (decode_static_host's 3D keys)."""
    return dict(boxes_3d=rec[:, :10].copy(), scores_3d=rec[:, 10].copy(), labels_3d=rec[:, 11].astype(np.int64),
                cls_scores=rec[:, 12].copy(), instance_ids=np.ascontiguousarray(rec[:, 13:15]).view(np.int64)[:, 0].copy())


def assert_same_annos(got, want, tracking):
    """Same boxes in the same order: names, attributes / ids and scores equal, floats within TOL."""
    assert len(got) == len(want), (len(got), len(want))
    exact = ("sample_token", "tracking_name", "tracking_id", "tracking_score") if tracking else \
        ("sample_token", "detection_name", "attribute_name", "detection_score")
    for i, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), (i, sorted(g), sorted(w))
        for k in exact:
            assert g[k] == w[k], (i, k, g[k], w[k])
        for k in ("translation", "size", "rotation", "velocity"):
            err = float(np.abs(np.asarray(g[k]) - np.asarray(w[k])).max())
            assert err <= TOL, (i, k, err)


def assert_records_equal(world, count, want_world, want_count):
    """A device record against the host's: counts equal, label / attribute / id lanes bit-equal, float lanes within TOL, pad rows
    exactly zero with label -1."""
    world, want_world = np.asarray(world), np.asarray(want_world)
    assert world.shape == want_world.shape and world.dtype == np.float64
    assert np.array_equal(np.asarray(count), np.asarray(want_count)), (count, want_count)
    assert np.array_equal(world[..., 13:16].view(np.int64), want_world[..., 13:16].view(np.int64))
    err = float(np.abs(world[..., :13] - want_world[..., :13]).max())
    print("max |device - host| over the float lanes:", err)
    assert err <= TOL, err
    pad = np.zeros(16)
    pad[13] = -1.0
    for s, n in enumerate(np.asarray(count)):
        rows = world[s, max(int(n), 0):]
        assert np.array_equal(rows.view(np.int64), np.broadcast_to(pad, rows.shape).copy().view(np.int64)), s
