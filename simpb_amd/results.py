"""Detection records -> nuScenes submission entries, on the host.

Restates datasets/nuscenes_dataset.py:504-586 (`_format_bbox`) with its helpers
`output_to_nusc_box` (:824-874) and `lidar_nusc_box_to_global` (:877-899) of the reference without
nuscenes-devkit / pyquaternion (absent here): quaternions are (w, x, y, z) numpy arrays. The class
ranges are those of nuscenes-devkit's `detection_cvpr_2019` config [third-party, restated: parity
unpinned -- the reference has no fixture for this step and the devkit is not in the container].
SURVEY.md §8(f) item 2."""
import json
import math

import numpy as np

DEFAULT_ATTRIBUTE = {  # nuscenes_dataset.py:26-37
    "car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked", "truck": "vehicle.parked",
    "bus": "vehicle.moving", "motorcycle": "cycle.without_rider", "construction_vehicle": "vehicle.parked",
    "bicycle": "cycle.without_rider", "barrier": "", "traffic_cone": "",
}
CLASS_RANGE = {  # detection_cvpr_2019
    "car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40, "motorcycle": 40,
    "bicycle": 40, "traffic_cone": 30, "barrier": 30,
}


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def quat_rotmat(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def yaw_quat(yaw):
    return np.array([math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)])


def format_sample(det, info, classes, tracking=False, threshold=None):
    """One sample's result dict (decoder.py:230-251 keys boxes_3d / scores_3d / labels_3d /
    cls_scores / instance_ids) -> list of nuScenes annotation dicts. `info` holds sample token,
    lidar2ego_{rotation,translation}, ego2global_{rotation,translation} (quaternions w,x,y,z)."""
    box3d = np.asarray(det["boxes_3d"], np.float64)
    scores = np.asarray(det["scores_3d"], np.float64)
    labels = np.asarray(det["labels_3d"]).astype(np.int64)
    ids = np.asarray(det["instance_ids"]).astype(np.int64) if "instance_ids" in det else None
    if threshold is not None:  # :830-838
        mask = (np.asarray(det["cls_scores"]) if "cls_scores" in det else scores) >= threshold
        box3d, scores, labels = box3d[mask], scores[mask], labels[mask]
        ids = ids[mask] if ids is not None else None
    l2e_q, l2e_t = np.asarray(info["lidar2ego_rotation"], np.float64), np.asarray(info["lidar2ego_translation"], np.float64)
    e2g_q, e2g_t = np.asarray(info["ego2global_rotation"], np.float64), np.asarray(info["ego2global_translation"], np.float64)
    r_l2e, r_e2g = quat_rotmat(l2e_q), quat_rotmat(e2g_q)
    annos = []
    for i in range(len(box3d)):
        name = classes[labels[i]]
        center = box3d[i, :3].copy()
        wlh = box3d[i, [4, 3, 5]]  # nus_box_dims = dims[:, [1, 0, 2]] (:849)
        quat = yaw_quat(box3d[i, 6])
        vel = np.array([box3d[i, 7], box3d[i, 8], 0.0])
        # lidar -> ego (:887-888)
        center, quat, vel = r_l2e @ center + l2e_t, quat_mul(l2e_q, quat), r_l2e @ vel
        if np.linalg.norm(center[:2]) > CLASS_RANGE[name]:  # :890-894
            continue
        # ego -> global (:896-897)
        center, quat, vel = r_e2g @ center + e2g_t, quat_mul(e2g_q, quat), r_e2g @ vel
        if tracking and name in ("barrier", "traffic_cone", "construction_vehicle"):
            continue
        if math.hypot(vel[0], vel[1]) > 0.2:  # :526-549
            if name in ("car", "construction_vehicle", "bus", "truck", "trailer"):
                attr = "vehicle.moving"
            elif name in ("bicycle", "motorcycle"):
                attr = "cycle.with_rider"
            else:
                attr = DEFAULT_ATTRIBUTE[name]
        else:
            attr = "pedestrian.standing" if name == "pedestrian" else ("vehicle.stopped" if name == "bus" else DEFAULT_ATTRIBUTE[name])
        anno = dict(sample_token=info["token"], translation=center.tolist(), size=wlh.tolist(), rotation=quat.tolist(),
                    velocity=vel[:2].tolist())
        if tracking:
            anno.update(tracking_name=name, tracking_score=float(scores[i]), tracking_id=str(int(ids[i])))
        else:
            anno.update(detection_name=name, detection_score=float(scores[i]), attribute_name=attr)
        annos.append(anno)
    return annos


def write_submission(results, infos, classes, path, modality=None, tracking=False, threshold=None, world_records=None):
    """results: list of per-sample dicts (or {'img_bbox': dict}); infos: matching list of sample infos.
    world_records: instead of `results` (which may then be None), one dict(record=, count=) per sample as the runners return
    it under res["img_bbox"]["world"]: already in the global frame, thresholded and range-limited (with the `tracking` and
    threshold the runner was built with), so only the dicts are written out."""
    out = {}
    if world_records is not None:
        for w, info in zip(world_records, infos):
            out[info["token"]] = annos_from_world(w["record"], w["count"], info["token"], classes, tracking)
        results = []
    for res, info in zip(results, infos):
        det = res.get("img_bbox", res)
        out[info["token"]] = format_sample(det, info, classes, tracking, threshold)
    sub = {"meta": modality or dict(use_lidar=False, use_camera=True, use_radar=False, use_map=False, use_external=False),
           "results": out}
    with open(path, "w") as f:
        json.dump(sub, f)
    return path


# ---- the world record: the same step for a whole frame at once, on the device (csrc/world.hip) or vectorised here
ATTRIBUTE_NAMES = ("", "vehicle.moving", "vehicle.parked", "vehicle.stopped", "cycle.with_rider", "cycle.without_rider",
                   "pedestrian.moving", "pedestrian.standing", "pedestrian.sitting_lying_down")
TRACKING_DROPPED = ("barrier", "traffic_cone", "construction_vehicle")
WORLD_WIDTH = 16        # translation 3 | size 3 | rotation 4 | velocity 2 | score | label | attribute code | track id (int64 bits)
WORLD_MAX_CLASSES = 32  # include/simpb_hip.h: SIMPB_WORLD_MAX_CLASSES
POSE_KEYS = ("lidar2ego_rotation", "lidar2ego_translation", "ego2global_rotation", "ego2global_translation")


def world_tables(classes, tracking):
    """The per-class tables of the world record from the class names: the range limit (negative = the class is never
    kept: what tracking mode does to barrier, traffic_cone and construction_vehicle) and the attribute codes (indices into
    ATTRIBUTE_NAMES) of a box that moves (speed above 0.2) and of one that does not: the rule of format_sample."""
    if len(classes) > WORLD_MAX_CLASSES:
        raise ValueError(f"{len(classes)} classes; the world record takes at most {WORLD_MAX_CLASSES}")
    rng = np.full(WORLD_MAX_CLASSES, -1.0, np.float32)
    moving, still = np.zeros(WORLD_MAX_CLASSES, np.uint8), np.zeros(WORLD_MAX_CLASSES, np.uint8)
    for c, name in enumerate(classes):
        rng[c] = -1.0 if tracking and name in TRACKING_DROPPED else CLASS_RANGE[name]
        if name in ("car", "construction_vehicle", "bus", "truck", "trailer"):
            m = "vehicle.moving"
        elif name in ("bicycle", "motorcycle"):
            m = "cycle.with_rider"
        else:
            m = DEFAULT_ATTRIBUTE[name]
        s = "pedestrian.standing" if name == "pedestrian" else ("vehicle.stopped" if name == "bus" else DEFAULT_ATTRIBUTE[name])
        moving[c], still[c] = ATTRIBUTE_NAMES.index(m), ATTRIBUTE_NAMES.index(s)
    return dict(class_range=rng, attr_moving=moving, attr_still=still)


def pose_row(info):
    """The four pose entries of a sample info as the record's pose row f64 [14], raw."""
    return np.concatenate([np.asarray(info[k], np.float64).reshape(-1) for k in POSE_KEYS])


def _rotmat_rows(q):
    w, x, y, z = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return ((1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)),
            (2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)),
            (2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)))


def world_record_host(rec3d, pose, tables, threshold, active=None):
    """csrc/world.hip in vectorised float64 numpy: rec3d f32 [streams, K, 15], pose f64 [streams, 14] (pose_row), tables from
    world_tables, threshold (None: no score cut), active (one flag per stream, or None) -> (world f64 [streams, K, 16],
    count i32 [streams]): the kept rows first, in rank order, zeros with label -1 behind them; count -1 and pad rows only for a
    stream that is not active."""
    rec = np.ascontiguousarray(np.asarray(rec3d, dtype=np.float32))
    streams, k, width = rec.shape
    if width != 15:
        raise ValueError(f"rec3d has {width} lanes, not 15")
    pose = np.asarray(pose, np.float64).reshape(streams, 14)
    world = np.zeros((streams, k, WORLD_WIDTH), np.float64)
    world[:, :, 13] = -1.0
    count = np.zeros(streams, np.int32)
    for s in range(streams):
        if active is not None and not active[s]:
            count[s] = -1
            continue
        r = rec[s][:, :13].astype(np.float64)   # (lanes 13:15 are id bits, not numbers)
        q1, t1, q2, t2 = pose[s, 0:4], pose[s, 4:7], pose[s, 7:11], pose[s, 11:14]
        m1, m2 = _rotmat_rows(q1), _rotmat_rows(q2)
        x, y, z, vx, vy = r[:, 0], r[:, 1], r[:, 2], r[:, 7], r[:, 8]
        c = [m1[i][0] * x + m1[i][1] * y + m1[i][2] * z + t1[i] for i in range(3)]
        u = [m1[i][0] * vx + m1[i][1] * vy for i in range(3)]
        cs, sn = np.cos(0.5 * r[:, 6]), np.sin(0.5 * r[:, 6])
        a = (q1[0] * cs - q1[3] * sn, q1[1] * cs + q1[2] * sn, q1[2] * cs - q1[1] * sn, q1[3] * cs + q1[0] * sn)
        label = rec[s][:, 11].astype(np.int64)
        known = (label >= 0) & (label < WORLD_MAX_CLASSES)
        idx = np.where(known, label, 0)
        rng = np.where(known, tables["class_range"][idx], np.float32(-1.0)).astype(np.float64)
        keep = (rng >= 0) & ~(np.sqrt(c[0] * c[0] + c[1] * c[1]) > rng)
        if threshold is not None:
            keep &= rec[s][:, 12] >= np.float32(threshold)
        g = [m2[i][0] * c[0] + m2[i][1] * c[1] + m2[i][2] * c[2] + t2[i] for i in range(3)]
        w = [m2[i][0] * u[0] + m2[i][1] * u[1] + m2[i][2] * u[2] for i in range(2)]
        bw, bx, by, bz = q2
        q = (bw * a[0] - bx * a[1] - by * a[2] - bz * a[3], bw * a[1] + bx * a[0] + by * a[3] - bz * a[2],
             bw * a[2] - bx * a[3] + by * a[0] + bz * a[1], bw * a[3] + bx * a[2] - by * a[1] + bz * a[0])
        code = np.where(np.hypot(w[0], w[1]) > 0.2, tables["attr_moving"][idx], tables["attr_still"][idx])
        row = np.stack([g[0], g[1], g[2], r[:, 4], r[:, 3], r[:, 5], q[0], q[1], q[2], q[3], w[0], w[1], r[:, 10],
                        label.astype(np.float64), code.astype(np.float64), np.zeros(k)], axis=1)
        row.view(np.int64)[:, 15] = np.ascontiguousarray(rec[s][:, 13:15]).view(np.int64)[:, 0]
        n = int(keep.sum())
        world[s, :n] = row[keep]
        count[s] = n
    return world, count


def annos_from_world(record, count, token, classes, tracking=False):
    """The list of annotation dicts format_sample returns, from one stream's world record (f64 [rows, 16], the first `count`
    rows are the boxes)."""
    record = np.asarray(record, np.float64)[:max(int(count), 0)]
    ids = np.ascontiguousarray(record[:, 15]).view(np.int64)
    annos = []
    for i, r in enumerate(record):
        name = classes[int(r[13])]
        anno = dict(sample_token=token, translation=r[0:3].tolist(), size=r[3:6].tolist(), rotation=r[6:10].tolist(),
                    velocity=r[10:12].tolist())
        if tracking:
            anno.update(tracking_name=name, tracking_score=float(r[12]), tracking_id=str(int(ids[i])))
        else:
            anno.update(detection_name=name, detection_score=float(r[12]), attribute_name=ATTRIBUTE_NAMES[int(r[14])])
        annos.append(anno)
    return annos
