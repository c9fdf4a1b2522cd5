"""Plain host model of the decoder's ranking, record and track-id operations (csrc/rowops.hip topk_rows, csrc/decode.hip,
csrc/bank.hip): numpy only, float64 arithmetic on fp32 inputs widened exactly, explicit loops where they read clearer.

Every ranking is "descending, ties to the lower index", stated as a two-key sort (score, then index). Every function returns
the discrete results together with the float64 scores they were derived from, so that a caller can check that the order was
decided by the mathematics (`assert_separated`) and not by how a device rounds an exponential.

Record columns as in include/simpb_hip.h: rec3d = x y z exp(w) exp(l) exp(h) yaw vx vy vz | score | label | score before the
re-score | id lanes (low, high); rec2d = x0 y0 x1 y1 | score | label | rank of the slot's anchor | camera."""
import numpy as np

ULP = 2.0 ** -23          # one fp32 ulp, relative
SEPARATION = 1e-5         # two scores the model ranks are bit-equal or further apart than this, relative


def f64(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x.astype(np.float64)


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def rank_desc(score, k):
    """Indices of the k largest entries of a 1-D float64 array: descending, ties to the lower index (-0.0 ties with +0.0)."""
    score = np.asarray(score, dtype=np.float64)
    order = np.lexsort((np.arange(score.shape[0]), -score))   # last key is the primary one
    return order[:k]


def assert_separated(scores, what=""):
    """The guard: any two of `scores` are bit-equal or differ by more than SEPARATION relative (in float64)."""
    v = np.unique(np.asarray(scores, dtype=np.float64).ravel())
    v = v[np.isfinite(v)]
    if v.size > 1:
        gap = np.diff(v) / np.maximum(np.abs(v[1:]), np.abs(v[:-1]))
        assert gap.min() > SEPARATION, (what, float(gap.min()))


# ------------------------------------------------------------------------------------------------------------------- top-k
def topk(scores, k):
    """scores f32 [bs, n] -> (index i64 [bs, k], values f64 [bs, k])."""
    s = f64(scores)
    index = np.stack([rank_desc(row, k) for row in s])
    return index, np.take_along_axis(s, index, 1)


# ------------------------------------------------------------------------------------------------------------------ decode
def class_score(cls):
    """cls f32 [..., C] -> (score f64 [...], label [...]): the maximum over classes of the sigmoid, and the first class that
    reaches it as fp32 sees the sigmoids (torch.max semantics on an fp32 tensor: every logit >= 17 is exactly 1.0f)."""
    s = sigmoid(f64(cls))
    return s.max(-1), np.argmax(s.astype(np.float32), -1)


def decode3d(cls, quality, box, ids, K):
    """cls f32 [bs, A, C], quality f32 [bs, A, 2] or None, box f32 [bs, A, 11], ids i64 [bs, A] or None."""
    bs, A, _ = cls.shape
    score0, label_of = class_score(cls)
    out = dict(score0=score0, anchor=np.zeros((bs, K), np.int64), label=np.zeros((bs, K), np.int64),
               score=np.zeros((bs, K)), column12=np.zeros((bs, K)), first=np.zeros((bs, K), np.int64),
               rank_of_anchor=np.full((bs, A), -1, np.int64), box=np.zeros((bs, K, 10)), raw_box=np.zeros((bs, K, 11), np.float32),
               lanes=np.zeros((bs, K, 2), np.uint32))
    for b in range(bs):
        first = rank_desc(score0[b], K)
        s = score0[b, first]
        if quality is not None:
            s = s * sigmoid(f64(quality)[b, first, 0])
        second = rank_desc(s, K)             # ties keep the first ranking's order: its positions are the index key
        anchor = first[second]
        out["first"][b], out["anchor"][b], out["score"][b] = first, anchor, s[second]
        out["label"][b] = label_of[b, anchor]
        out["column12"][b] = score0[b, first]        # NOT re-ordered by the second ranking (decoder.py:157-167)
        out["rank_of_anchor"][b, anchor] = np.arange(K)
        bx = f64(box)[b, anchor]
        out["raw_box"][b] = box[b, anchor]
        out["box"][b] = np.concatenate([bx[:, 0:3], np.exp(bx[:, 3:6]), np.arctan2(bx[:, 6], bx[:, 7])[:, None], bx[:, 8:11]], 1)
        kept = ids[b, anchor] if ids is not None else np.full(K, -1, np.int64)
        u = kept.astype(np.int64).view(np.uint64)
        out["lanes"][b, :, 0], out["lanes"][b, :, 1] = (u & 0xFFFFFFFF).astype(np.uint32), (u >> 32).astype(np.uint32)
    return out


def _pixels(box2d, crop, resize):
    """decode_box2d (decoder.py:36-51): cxcywh in crop units -> xyxy pixels of the original image. `resize` is the fp32 the
    entry point receives."""
    b = f64(box2d)
    cw, ch, y0, rs = float(crop[2] - crop[0]), float(crop[3] - crop[1]), float(crop[1]), float(np.float32(resize))
    cx, cy, w, h = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([np.clip((cx - 0.5 * w) * cw, 0, cw) / rs, (np.clip((cy - 0.5 * h) * ch, 0, ch) + y0) / rs,
                     np.clip((cx + 0.5 * w) * cw, 0, cw) / rs, (np.clip((cy + 0.5 * h) * ch, 0, ch) + y0) / rs], -1)


def decode2d(cls2d, box2d, q2a, query_cam, rank_of_anchor, crop, resize):
    """cls2d f32 [bs, N2, C], box2d f32 [bs, N2, 4], q2a i32 [bs, N2] (anchor within the stream, -1 or out of range: no
    anchor), query_cam i32 [N2], rank_of_anchor [bs, A] -> rec f64 [bs, N2, 8]."""
    bs, N2, _ = cls2d.shape
    A = rank_of_anchor.shape[1]
    rec = np.zeros((bs, N2, 8))
    rec[..., 0:4] = _pixels(box2d, crop, resize)
    rec[..., 4], rec[..., 5] = class_score(cls2d)
    for b in range(bs):
        for i in range(N2):
            a = int(q2a[b, i])
            rec[b, i, 6] = rank_of_anchor[b, a] if 0 <= a < A else -1
            rec[b, i, 7] = query_cam[i]
    return rec


def decode2d_ragged(cls2d, box2d, q2a, query_cam, group_start, rank_of_anchor, rows, cams, crop, resize):
    """The flat, stream-major slot array of a batch of independent streams: cls2d f32 [S, C], box2d f32 [S, 4], q2a i32 [S]
    (flat anchor b * A + a), query_cam i32 [S] (flat group b * cams + cam), group_start i32 [bs * cams + 1] -> rec f64
    [bs, rows, 8]: a stream's first `rows` slots in its leading rows, pad rows (zeros, rank -1, camera -1) behind."""
    bs = rank_of_anchor.shape[0]
    flat = rank_of_anchor.reshape(-1)
    px = _pixels(box2d, crop, resize)
    score, label = class_score(cls2d)
    rec = np.zeros((bs, rows, 8))
    rec[..., 6:8] = -1
    for b in range(bs):
        lo, hi = int(group_start[b * cams]), int(group_start[(b + 1) * cams])
        for r in range(min(rows, hi - lo)):
            j = lo + r
            a = int(q2a[j])
            rec[b, r, 0:4], rec[b, r, 4], rec[b, r, 5] = px[j], score[j], label[j]
            rec[b, r, 6] = flat[a] if 0 <= a < flat.shape[0] else -1
            rec[b, r, 7] = int(query_cam[j]) - b * cams
    return rec


# -------------------------------------------------------------------------------------------------------------------- bank
def bank_get(anchor, T_temp2cur, dt, max_dt, default_dt):
    """instance_bank.py:83-113. anchor f32 [bs, n, 11], T f32 [bs, 4, 4], dt f32 [bs] -> dict(anchor f64 [bs, n, 11], size f64
    (the sum of the magnitudes of the terms of every column: what a rounding error is relative to), mask, dt f32)."""
    a, m, t = f64(anchor), f64(T_temp2cur), f64(dt)
    limit = float(np.float32(max_dt))
    mask = np.abs(t) <= limit
    dt_out = np.where((t != 0) & mask, dt, np.float32(default_dt)).astype(np.float32)
    out, size = np.zeros(a.shape), np.zeros(a.shape)
    for b in range(a.shape[0]):
        R, tr = m[b, :3, :3], m[b, :3, 3]
        vel = a[b, :, 8:11]
        centre = a[b, :, 0:3] + vel * t[b]        # anchor_projection(..., time_intervals=[-dt]): c - v * (-dt)
        out[b, :, 0:3] = centre @ R.T + tr
        size[b, :, 0:3] = (np.abs(a[b, :, 0:3]) + np.abs(vel * t[b])) @ np.abs(R.T) + np.abs(tr)
        out[b, :, 3:6] = a[b, :, 3:6]
        cs = a[b][:, [7, 6]]                      # the 2x2 block applied to [cos, sin], stored into the [sin, cos] slots
        out[b, :, 6:8] = cs @ R[:2, :2].T
        size[b, :, 6:8] = np.abs(cs) @ np.abs(R[:2, :2].T)
        out[b, :, 8:11] = vel @ R.T
        size[b, :, 8:11] = np.abs(vel) @ np.abs(R.T)
    return dict(anchor=out, size=size, mask=mask, dt=dt_out)


def bank_update(cls, cur_f, cur_a, cached_f, cached_a, mask, ids):
    """instance_bank.py:121-150: [cached T | the A - T best current by maximum raw logit] for streams under `mask`, the
    current rows as they are for the others, whose ids are reset. Rows are copies: same dtype out as in."""
    bs, A, _ = cls.shape
    T = cached_f.shape[1]
    key = f64(cls).max(-1)
    index = np.stack([rank_desc(key[b], A - T) for b in range(bs)])
    out_f, out_a, ids = cur_f.copy(), cur_a.copy(), ids.copy()
    for b in range(bs):
        if mask[b]:
            out_f[b] = np.concatenate([cached_f[b], cur_f[b, index[b]]])
            out_a[b] = np.concatenate([cached_a[b], cur_a[b, index[b]]])
        else:
            ids[b] = -1
    return dict(index=index, key=key, feature=out_f, anchor=out_a, ids=ids)


def bank_commit(state, cls, feature, anchor, has_prev, threshold=None, active=None, decay=0.6):
    """instance_bank.py:152-196 on state = dict(conf f32 [bs, T], feature [bs, T, E], anchor [bs, T, 11], ids i64 [bs, A],
    prev_id int). Returns (new state, dict(ids i64 [bs, A], index [bs, T], kept f64 [bs, T], ranked f64 [bs, A], fresh f64
    [bs, A])). The new confidences are kept as the fp32 nearest to the float64 result, like every other fp32 input."""
    bs, A, _ = cls.shape
    T = state["conf"].shape[1]
    new = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    fresh_score = sigmoid(f64(cls).max(-1))
    ranked = fresh_score.copy()
    out = dict(ids=np.full((bs, A), -1, np.int64), index=np.full((bs, T), -1, np.int64), kept=np.zeros((bs, T)), ranked=ranked,
               fresh=fresh_score)
    next_id = int(state["prev_id"])
    for b in range(bs):
        if active is not None and not active[b]:
            continue
        if has_prev:
            ranked[b, :T] = np.maximum(f64(state["conf"])[b] * float(np.float32(decay)), fresh_score[b, :T])
        index = rank_desc(ranked[b], T)
        ids = state["ids"][b].copy()
        for a in range(A):     # stream-major, anchor-ascending numbering over the flattened batch
            if ids[a] < 0 and (threshold is None or fresh_score[b, a] >= float(np.float32(threshold))):
                ids[a] = next_id
                next_id += 1
        out["ids"][b], out["index"][b], out["kept"][b] = ids, index, ranked[b, index]
        new["conf"][b] = ranked[b, index].astype(np.float32)
        new["feature"][b], new["anchor"][b] = feature[b, index], anchor[b, index]
        new["ids"][b] = -1
        new["ids"][b, :T] = ids[index]
    new["prev_id"] = next_id
    return new, out
