"""Plain host model of the query allocation and the index moves built on it (csrc/alloc.hip): numpy only, float64 arithmetic
on fp32 inputs widened exactly, explicit loops where they read clearer. Nothing here imports from simpb_amd.plugin.

`project` transcribes allocation.py:29-83 of the reference point by point: nine points per (stream, anchor, camera) -- the
eight corners of the size-clamped box in np.unravel_index order, then the centre -- projected, divided by max(d, 1e-5) and
tested against the image border (strict inequalities) and, for the corners only, against d > 0. `tables` lays the flagged
pairs out as the reference does (allocation.py:89-143, index form), as the static-capacity cut of that layout, and as the
flat stream-major layout of a batch of independent streams. `gather` and `aggregate` are simpb_head.py:438 and
aggregation.py:23-35.

The 1e-5 of both clamps is the float32 nearest to 1e-5 (what torch.clamp(1e-5) on a float32 tensor and the kernels' 1e-5f
compare with), widened; it differs from the decimal by 3.6e-9 relative.

Whether a pair is flagged is a discrete answer, so a caller has to know that it was decided by the mathematics and not by how
a device rounds a product. Every tested quantity therefore carries a *size*: the sum of the magnitudes of the terms it is
summed from (for u, v, d the twelve-or-fewer products P[r, k] * (box term) and P[r, 3]; for x = u / dc and y = v / dc that
sum divided by dc), and UNIT * size = 2^-24 * size is what one float32 rounding of it can move. The *margin* of a quantity is
its distance to the value it is compared with (x to 0 and img_w, y to 0 and img_h, d to 0) in those units; a pair is decided
when every one of its 27 margins (nine points, x / y / d) is at least DECIDED = 64: u, v and d are four products and three
additions each on operands that carry three to four roundings themselves, then one division -- under twenty roundings in any
evaluation order, fused or not, each at most one unit. `assert_decided` raises with the offending pairs; its `waive` mask
takes out exactly the quantities a caller has proven to be computed without any rounding (`exact_quantities`), and counts
an x or y that is the one division of two such numbers in roundings of the quotient alone (`waived_margins`)."""
import numpy as np

UNIT = 2.0 ** -24           # half a float32 ulp, relative: one rounding
DECIDED = 64.0              # margins in units of UNIT * size (module docstring)
CLAMP = float(np.float32(1e-5))
LIMITS = (35.0, 35.0, 10.0)
CORNERS = np.stack(np.unravel_index(np.arange(8), [2] * 3), axis=1) - 0.5     # [8, 3], allocation.py:43-44


def f64(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x.astype(np.float64)


# --------------------------------------------------------------------------------------------------------------- projection
def project(anchor, proj, img_wh, limits=LIMITS, active=None, cam_valid=None, dtype=np.float64):
    """anchor f32 [bs, A, 11], proj f32 [bs, cams, 4, 4] -> dict, everything in the kernels' [bs, cams, A] order:
      flag u8 (0 none / 1 a corner only / 2 the centre), sel [.., 2] the selected pixel, depth the centre's SIGNED d,
      size_sel [.., 2] / size_depth their sizes, x / y / d [.., 9] every point, margin_q [.., 9, 3] and margin [..] = its
      minimum per pair. active (bs) / cam_valid (bs, cams): a 0 gives flag 0 and zeros whatever the inputs hold (the kernel's
      early exit), with an infinite margin. dtype=np.float32 evaluates the same statements in float32 (one rounding per
      operation, no fused multiply-add): only `exact_quantities` uses that."""
    T = dtype
    assert np.asarray(anchor).dtype == np.float32 and np.asarray(proj).dtype == np.float32
    an, P = np.asarray(anchor).astype(T), np.asarray(proj).astype(T)
    bs, A, _ = an.shape
    cams = P.shape[1]
    w, h = T(img_wh[0]), T(img_wh[1])
    with np.errstate(all="ignore"):
        size = np.minimum(np.exp(an[..., 3:6]), np.asarray(limits, T))            # allocation.py:46-47
        off = size[:, :, None, :] * CORNERS.astype(T)[None, None]                  # [bs, A, 8, 3]
        sn, cs = an[..., 6:7], an[..., 7:8]
        c3 = an[..., None, 0:3]                                                    # [bs, A, 1, 3]
        ox, oy, oz = off[..., 0], off[..., 1], off[..., 2]
        corners = np.stack([(cs * ox - sn * oy) + c3[..., 0], (sn * ox + cs * oy) + c3[..., 1], oz + c3[..., 2]], -1)
        mags = np.stack([np.abs(cs * ox) + np.abs(sn * oy) + np.abs(c3[..., 0]),
                         np.abs(sn * ox) + np.abs(cs * oy) + np.abs(c3[..., 1]), np.abs(oz) + np.abs(c3[..., 2])], -1)
        pts = np.concatenate([corners, c3], 2)[:, None]                            # [bs, 1, A, 9, 3], the centre last (:52)
        mags = np.concatenate([mags, np.abs(c3)], 2)[:, None]
        Pm = P[:, :, None, None]                                                   # [bs, cams, 1, 1, 4, 4]

        def row(r):
            val = ((Pm[..., r, 0] * pts[..., 0] + Pm[..., r, 1] * pts[..., 1]) + Pm[..., r, 2] * pts[..., 2]) + Pm[..., r, 3]
            mag = (np.abs(Pm[..., r, 0]) * mags[..., 0] + np.abs(Pm[..., r, 1]) * mags[..., 1]
                   + np.abs(Pm[..., r, 2]) * mags[..., 2] + np.abs(Pm[..., r, 3]))
            return val, mag                                                        # [bs, cams, A, 9]

        (u, su), (v, sv), (d, sd) = row(0), row(1), row(2)
        dc = np.maximum(d, T(np.float32(1e-5)))                                    # :64-65
        x, y, sx, sy = u / dc, v / dc, su / dc, sv / dc
        inside = (0 < x) & (x < w) & (0 < y) & (y < h)                             # :67-72, strict
        center_valid = inside[..., 8]                                              # no depth test on the centre
        corner_valid = ((d[..., :8] > 0) & inside[..., :8]).any(-1)

        def mid(val, siz, top):                                                    # :76-81
            lo, hi = val[..., :8].argmin(-1)[..., None], val[..., :8].argmax(-1)[..., None]
            m = (np.clip(np.take_along_axis(val, lo, -1), 0, top) + np.clip(np.take_along_axis(val, hi, -1), 0, top)) / T(2)
            s = np.maximum(np.take_along_axis(siz, lo, -1), np.take_along_axis(siz, hi, -1))
            return m[..., 0], np.maximum(s[..., 0], np.abs(m[..., 0]))

        (mx, smx), (my, smy) = mid(x, sx, w), mid(y, sy, h)
        sel = np.stack([np.where(center_valid, x[..., 8], mx), np.where(center_valid, y[..., 8], my)], -1)
        size_sel = np.stack([np.where(center_valid, sx[..., 8], smx), np.where(center_valid, sy[..., 8], smy)], -1)
        flag = np.where(center_valid, 2, np.where(corner_valid, 1, 0)).astype(np.uint8)

        def margin(dist, siz):
            return np.where(dist == 0, 0.0, dist.astype(np.float64) / np.maximum(UNIT * siz.astype(np.float64), 1e-300))

        margin_q = np.stack([margin(np.minimum(np.abs(x), np.abs(x - w)), sx), margin(np.minimum(np.abs(y), np.abs(y - h)), sy),
                             margin(np.abs(d), sd)], -1)
        # the same distances where u, v and d carry no rounding at all: only the division rounds, by at most UNIT * |x|
        margin_div = np.stack([margin(np.minimum(np.abs(x), np.abs(x - w)), np.abs(x)),
                               margin(np.minimum(np.abs(y), np.abs(y - h)), np.abs(y))], -1)
    depth, size_depth = d[..., 8], sd[..., 8]
    off_pair = np.zeros((bs, cams), bool)
    if active is not None:
        off_pair |= ~np.asarray(active, bool).reshape(bs, 1)
    if cam_valid is not None:
        off_pair |= ~np.asarray(cam_valid, bool).reshape(bs, cams)
    o = off_pair[..., None]
    z = T(0)
    out = dict(flag=np.where(o, 0, flag).astype(np.uint8), sel=np.where(o[..., None], z, sel), depth=np.where(o, z, depth),
               size_sel=np.where(o[..., None], z, size_sel), size_depth=np.where(o, z, size_depth), x=x, y=y, d=d, u=u, v=v,
               margin_q=np.where(o[..., None, None], np.inf, margin_q), margin_div=margin_div)
    out["margin"] = out["margin_q"].min((-1, -2))
    return out


def exact_quantities(anchor, proj, img_wh, limits=LIMITS):
    """bool [bs, cams, A, 9, 5]: the x / y / d / u / v that the statements evaluated in float32 give with the float64 value,
    bit for bit after widening -- no operation on the way rounded, so no evaluation order and no fused multiply-add can give
    another float32. (The centre's and the corners' projections of dyadic inputs through a power-of-two pinhole.)"""
    a, b = project(anchor, proj, img_wh, limits), project(anchor, proj, img_wh, limits, dtype=np.float32)
    return np.stack([b[k].astype(np.float64) == a[k] for k in ("x", "y", "d", "u", "v")], -1)


def waived_margins(p, waive):
    """margin_q [.., 9, 3] with what `waive` (exact_quantities) proves taken out: an exact x, y or d is infinitely far from
    every threshold; an x (y) that is the one division of an exact u (v) by an exact d carries that division's rounding only,
    so its distance counts in units of |x| (|y|)."""
    m = p["margin_q"].copy()
    for q, top in ((0, 3), (1, 4)):
        m[..., q] = np.where(waive[..., top] & waive[..., 2], p["margin_div"][..., q], m[..., q])
    return np.where(waive[..., :3], np.inf, m)


def undecided(p, waive=None):
    """[(stream, anchor, camera, margin)] of the pairs with a margin under DECIDED among the quantities not waived."""
    m = p["margin_q"] if waive is None else waived_margins(p, waive)
    pair = m.min((-1, -2))
    return [(int(b), int(a), int(c), float(pair[b, c, a])) for b, c, a in np.argwhere(pair < DECIDED)]


def assert_decided(p, waive=None, what=""):
    bad = undecided(p, waive)
    assert not bad, f"{what}: {len(bad)} undecided (stream, anchor, camera, margin): {bad[:8]}"


# ------------------------------------------------------------------------------------------------------------------- tables
def compact(flag):
    """count i32 [bs, cams] and, per (stream, camera), the flagged anchors in ascending order (allocation.py:103-108)."""
    bs, cams, _ = flag.shape
    order = [[np.flatnonzero(flag[b, c]) for c in range(cams)] for b in range(bs)]
    return np.asarray([[len(o) for o in row] for row in order], np.int32), order


def group_table(count, capacity=None):
    """(group_start [cams + 1], overflow): prefix sums of the maximum over the batch of every camera's count
    (allocation.py:91-94), cut at `capacity` where one is given."""
    cum = np.concatenate([[0], np.cumsum(np.asarray(count, np.int64).max(0))])
    if capacity is None:
        return cum.astype(np.int32), 0
    return np.minimum(cum, capacity).astype(np.int32), int(cum[-1] > capacity)


def tables(flag, sel, depth, img_wh, form="exact", capacity=None, size_sel=None, size_depth=None):
    """flag u8 [bs, cams, A], sel [bs, cams, A, 2], depth [bs, cams, A] as `project` returns them.
      form "exact":  the reference's layout, N2 = the sum over cameras of the maximum count over the batch; a stream with fewer
                     flagged anchors in a camera than that has pads (q2a -1, zeros) at the end of that group;
      form "static": that layout cut at `capacity` slots: slots past the cut do not exist (their anchors' a2q stays -1),
                     query_cam is -1 past the last group, overflow says whether anything was cut;
      form "ragged": a batch of independent streams as ONE flat slot array of bs * capacity slots, stream-major then
                     camera-major without pads, at most `capacity` slots per stream (more: overflow, cut), q2a the flat
                     anchor index b * A + a, query_cam the group b * cams + cam, group_start over bs * cams groups.
    Returns count, order (lists), group_start, overflow, q2a, is_center, a2q [bs, A, cams], query_cam, ref_pts2d (f64, sel /
    (img_w, img_h)), ref_depth2d (f64, |depth|), size_pts / size_depth (when given); slot arrays are [bs, N2] ("ragged":
    [1, bs * capacity])."""
    bs, cams, A = flag.shape
    wh = np.asarray(img_wh, np.float64)
    count, order = compact(flag)
    if form == "ragged":
        rows, n2 = 1, bs * capacity
    else:
        group_start, overflow = group_table(count, capacity if form == "static" else None)
        rows, n2 = bs, int(capacity if form == "static" else group_start[-1])
    t = dict(count=count, order=order, q2a=np.full((rows, n2), -1, np.int32), is_center=np.zeros((rows, n2), np.int32),
             a2q=np.full((bs, A, cams), -1, np.int32), query_cam=np.full(n2, -1, np.int32), ref_pts2d=np.zeros((rows, n2, 2)),
             ref_depth2d=np.zeros((rows, n2)), size_pts=np.zeros((rows, n2, 2)), size_depth=np.zeros((rows, n2)))

    def put(row, slot, b, c, a, index):
        t["q2a"][row, slot] = index
        t["is_center"][row, slot] = int(flag[b, c, a] == 2)
        t["a2q"][b, a, c] = slot
        t["ref_pts2d"][row, slot] = sel[b, c, a] / wh                              # allocation.py:125
        t["ref_depth2d"][row, slot] = abs(depth[b, c, a])                          # :123
        if size_sel is not None:
            t["size_pts"][row, slot] = size_sel[b, c, a] / wh
            t["size_depth"][row, slot] = size_depth[b, c, a]

    if form == "ragged":
        start, overflow, pos = [0], 0, 0
        for b in range(bs):
            room = capacity
            for c in range(cams):
                take = min(len(order[b][c]), room)
                overflow |= int(len(order[b][c]) > room)
                for r in range(take):
                    put(0, pos + r, b, c, order[b][c][r], b * A + order[b][c][r])
                t["query_cam"][pos:pos + take] = b * cams + c
                pos, room = pos + take, room - take
                start.append(pos)
        group_start = np.asarray(start, np.int32)
    else:
        for c in range(cams):
            lo, hi = int(group_start[c]), int(group_start[c + 1])
            t["query_cam"][lo:hi] = c
            for b in range(bs):
                for r, a in enumerate(order[b][c][:hi - lo]):
                    put(b, lo + r, b, c, a, a)
    t.update(group_start=group_start, overflow=overflow, n2=n2)
    return t


# -------------------------------------------------------------------------------------------------------------- index moves
def gather(src, q2a):
    """out[b, s] = src[b, q2a[b, s]], zeros where q2a < 0 (simpb_head.py:438 without the one-hot matrix); src's own dtype."""
    out = np.zeros(q2a.shape + src.shape[2:], src.dtype)
    for b in range(q2a.shape[0]):
        live = q2a[b] >= 0
        out[b, live] = src[b, q2a[b, live]]
    return out


def aggregate(q3d, pos3d, q2d, pos2d, q2a, alpha=None, hidden=None, weight=None, bias=None):
    """aggregation.py:23-35 with the one-hot matrix built from q2a [bs, N2] (trans[b, s, q2a[b, s]] = 1): alpha f32 [bs, N2]
    given, or sigmoid(hidden . weight + bias). Returns out_q, out_pos (q3d + sum alpha q2d / max(sum alpha, 1e-5)), their sizes
    (|q3d| + sum |alpha q2d| / the divisor) and the unclamped sums of alpha [bs, A]. In the hidden form a rounding of the
    logit, of size sum |hidden weight| + |bias|, moves alpha by (1 - alpha) times that, relative, and a quotient of two sums
    over alpha by at most twice that: the 2D term of the size is multiplied by 1 + 2 * the largest logit size among the
    anchor's slots."""
    q3d, pos3d, q2d, pos2d = f64(q3d), f64(pos3d), f64(q2d), f64(pos2d)
    bs, A, _ = q3d.shape
    n2 = q2d.shape[1]
    logit_size = np.zeros((bs, n2))
    if alpha is None:
        logit = f64(hidden) @ f64(weight) + (float(bias) if bias is not None else 0.0)
        logit_size = np.abs(f64(hidden)) @ np.abs(f64(weight)) + (abs(float(bias)) if bias is not None else 0.0)
        with np.errstate(over="ignore"):
            alpha = 1.0 / (1.0 + np.exp(-logit))
    else:
        alpha = f64(alpha).reshape(bs, n2)
    trans = np.zeros((bs, n2, A))
    for b in range(bs):
        live = np.flatnonzero(q2a[b] >= 0)
        trans[b, live, q2a[b, live]] = 1.0
    rw = (trans * alpha[..., None]).transpose(0, 2, 1)                              # :32
    total = rw.sum(-1, keepdims=True)
    div = np.maximum(total, CLAMP)                                                 # :33
    out_q, out_pos = q3d + rw @ q2d / div, pos3d + rw @ pos2d / div                # :34-35 and the residual (:88-89)
    wide = 1.0 + 2.0 * (trans.transpose(0, 2, 1) * logit_size[:, None, :]).max(-1, keepdims=True)
    return (out_q, out_pos, np.abs(q3d) + wide * (rw @ np.abs(q2d)) / div, np.abs(pos3d) + wide * (rw @ np.abs(pos2d)) / div,
            total[..., 0])
