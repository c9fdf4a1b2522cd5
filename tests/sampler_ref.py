"""The deformable samplers stated in float64, tap by tap (numpy only; nothing of the package under test is imported).

  daf            3D deformable aggregation (csrc/deform_agg.hip, csrc/deform_agg_fused.hip)
  msda           multi-scale deformable attention = grid_sample(bilinear, zeros, align_corners=False) written out
  msda_linear    the 2176-wide row of csrc/msda_lin.hip: softmax, reference point + offset, the two brackets
  dfa_points     key points -> projection -> sampling locations (csrc/dfa_prep.hip)
  dfa_weights    softmax of feat_logits + cam_logits over cams * L * P per group

Locations, offsets and logits are taken as the fp32 numbers the kernels are given and widened exactly; every operation
after that is float64. Each sampler also returns, per output element,
  abs_sum   the same sum with every product replaced by its absolute value, and
  grad_sum  sum over samples of |w_s| * (eps_x + eps_y) * 2 * max|v|, eps = 2^-23 * (|loc| * size + 0.5): what the fp32
            rounding of `loc * size - 0.5` can move a bilinear patch by (slope <= 2 max|v| per pixel).
max|v| runs over the sample's in-map taps; where the float64 pixel lies within eps of an integer the fp32 pixel may floor
into the neighbouring cell, so the row / column of taps beyond that integer counts too (bilinear interpolation with zero
padding is continuous there, but its slope on the other side is set by those taps)."""
import numpy as np

EPS_PIX = 2.0 ** -23


def f64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def _i64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.int64)


def _sample(fmap, bi, px, py, ex, ey):
    """fmap [B, H, W, C]; sample s reads map bi[s] at pixel (px[s], py[s]) -> (val [n, C], abs [n, C], vmax [n, C],
    wsum [n]): the four taps, each zero outside the map; a non-finite or far-away pixel has no tap inside."""
    _, H, W, C = fmap.shape
    n = px.shape[0]
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(px) & np.isfinite(py) & (px > -1) & (px < W) & (py > -1) & (py < H)
    px, py = np.where(fin, px, 0.0), np.where(fin, py, 0.0)
    x0, y0 = np.floor(px), np.floor(py)
    lx, ly = px - x0, py - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    val, ab, vmax, wsum = np.zeros((n, C)), np.zeros((n, C)), np.zeros((n, C)), np.zeros(n)
    wy = {0: 1.0 - ly, 1: ly}
    wx = {0: 1.0 - lx, 1: lx}
    near_y = {-1: ly <= ey, 2: (1.0 - ly) <= ey}
    near_x = {-1: lx <= ex, 2: (1.0 - lx) <= ex}
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            yy, xx = y0 + dy, x0 + dx
            ok = fin & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            if dy in (0, 1) and dx in (0, 1):
                v = fmap[bi, yy.clip(0, H - 1), xx.clip(0, W - 1)]
                w = np.where(ok, wy[dy] * wx[dx], 0.0)
                val += w[:, None] * np.where(ok[:, None], v, 0.0)
                ab += w[:, None] * np.where(ok[:, None], np.abs(v), 0.0)
                vmax = np.maximum(vmax, np.where(ok[:, None], np.abs(v), 0.0))
                wsum += w
            else:
                inc = ok & near_y.get(dy, True) & near_x.get(dx, True)
                if inc.any():
                    i = np.nonzero(inc)[0]
                    vmax[i] = np.maximum(vmax[i], np.abs(fmap[bi[i], yy[i], xx[i]]))
    return val, ab, vmax, wsum


def _pixel(loc, size):
    """float64 pixel coordinate and eps of a normalised coordinate (fp32 numbers widened)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return loc * size - 0.5, EPS_PIX * (np.abs(loc) * size + 0.5)


def daf(feat, spatial_shape, scale_start, loc, weights):
    """feat [bs, N, C]; spatial_shape [cams, L, 2] = (H, W); scale_start [cams, L]; loc fp32 [bs, A, P, cams, 2] = (x, y);
    weights [bs, A, P, cams, L, G] -> (out, abs_sum, grad_sum), each float64 [bs, A, C]. A sample counts only when
    0 < x < 1 and 0 < y < 1 on the fp32 values; channel c uses group c // (C / G)."""
    feat, w = f64(feat), f64(weights)
    ss, st = _i64(spatial_shape), _i64(scale_start)
    loc32 = np.asarray(loc.detach().cpu().numpy() if hasattr(loc, "detach") else loc, dtype=np.float32)
    bs, _, C = feat.shape
    A, P, cams = loc32.shape[1:4]
    L, G = ss.shape[1], w.shape[-1]
    with np.errstate(invalid="ignore"):
        keep = (loc32[..., 0] > 0) & (loc32[..., 0] < 1) & (loc32[..., 1] > 0) & (loc32[..., 1] < 1)
    loc = loc32.astype(np.float64)
    out, ab, gr = (np.zeros((bs * A, C)) for _ in range(3))
    for cam in range(cams):
        b, a, p = np.nonzero(keep[:, :, :, cam])
        if b.size == 0:
            continue
        x, y = loc[b, a, p, cam, 0], loc[b, a, p, cam, 1]
        s_val, s_ab, s_gr = (np.zeros((b.size, C)) for _ in range(3))
        for lvl in range(L):
            H, W, start = int(ss[cam, lvl, 0]), int(ss[cam, lvl, 1]), int(st[cam, lvl])
            fmap = feat[:, start:start + H * W].reshape(bs, H, W, C)
            (px, ex), (py, ey) = _pixel(x, W), _pixel(y, H)
            val, aval, vmax, _ = _sample(fmap, b, px, py, ex, ey)
            wg = np.repeat(w[b, a, p, cam, lvl], C // G, axis=-1)
            s_val += wg * val
            s_ab += np.abs(wg) * aval
            s_gr += np.abs(wg) * ((ex + ey) * 2.0)[:, None] * vmax
        rows = b * A + a                      # ascending: np.nonzero walks (b, a, p) in order
        first = np.nonzero(np.diff(rows, prepend=-1))[0]
        for dst, src in ((out, s_val), (ab, s_ab), (gr, s_gr)):
            dst[rows[first]] += np.add.reduceat(src, first, axis=0)
    return out.reshape(bs, A, C), ab.reshape(bs, A, C), gr.reshape(bs, A, C)


def _msda(value, shapes, loc, attn):
    """value [bs, Nv, heads, hd]; loc [bs, nq, heads, L, P, 2]; attn [bs, nq, heads, L, P] (float64 already) ->
    (out, abs_sum, grad_sum [bs, nq, heads, hd], wsum [bs, nq, heads] = sum of attn * valid tap weights)."""
    bs, _, heads, hd = value.shape
    nq, _, L, P = loc.shape[1:5]
    out, ab, gr = (np.zeros((bs, nq, heads, hd)) for _ in range(3))
    ws = np.zeros((bs, nq, heads))
    bi = np.repeat(np.arange(bs), nq * P)
    start = 0
    for lvl in range(L):
        H, W = int(shapes[lvl][0]), int(shapes[lvl][1])
        for h in range(heads):
            fmap = value[:, start:start + H * W, h].reshape(bs, H, W, hd)
            (px, ex), (py, ey) = _pixel(loc[:, :, h, lvl, :, 0].reshape(-1), W), _pixel(loc[:, :, h, lvl, :, 1].reshape(-1), H)
            ex, ey = np.where(np.isfinite(ex), ex, 0.0), np.where(np.isfinite(ey), ey, 0.0)
            val, aval, vmax, wsum = _sample(fmap, bi, px, py, ex, ey)
            a = attn[:, :, h, lvl].reshape(-1)
            out[:, :, h] += (a[:, None] * val).reshape(bs, nq, P, hd).sum(2)
            ab[:, :, h] += (np.abs(a)[:, None] * aval).reshape(bs, nq, P, hd).sum(2)
            gr[:, :, h] += ((np.abs(a) * (ex + ey) * 2.0)[:, None] * vmax).reshape(bs, nq, P, hd).sum(2)
            ws[:, :, h] += (a * wsum).reshape(bs, nq, P).sum(2)
        start += H * W
    return out, ab, gr, ws


def msda(value, shapes, loc, attn):
    """value [bs, Nv, heads, hd]; shapes [(H, W)] * L; loc fp32 [bs, nq, heads, L, P, 2] = (x, y) normalised;
    attn [bs, nq, heads, L, P] -> (out, abs_sum, grad_sum), each float64 [bs, nq, heads * hd]. pixel = loc * size - 0.5,
    four taps, each zero outside the map."""
    value, loc, attn = f64(value), f64(loc), f64(attn)
    shapes = _i64(shapes)
    out, ab, gr, _ = _msda(value, shapes, loc, attn)
    bs, nq = out.shape[:2]
    return out.reshape(bs, nq, -1), ab.reshape(bs, nq, -1), gr.reshape(bs, nq, -1)


HEADS, LVLS, PTS, CH, ROW = 8, 4, 4, 256, 8 * 256 + 128


def msda_offsets(raw, ref, shapes):
    """(loc [bs, nq, 8, 4, 4, 2], attn [bs, nq, 8, 4, 4]) of a [offsets 256 | logits 128] row: softmax over the 16 logits of
    a head, ref + offset / (W_l, H_l)."""
    raw, ref, shapes = f64(raw), f64(ref), _i64(shapes)
    bs, nq = raw.shape[:2]
    off = raw[..., :2 * HEADS * LVLS * PTS].reshape(bs, nq, HEADS, LVLS, PTS, 2)
    lg = raw[..., 2 * HEADS * LVLS * PTS:].reshape(bs, nq, HEADS, LVLS * PTS)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    attn = (e / e.sum(-1, keepdims=True)).reshape(bs, nq, HEADS, LVLS, PTS)
    norm = np.stack([shapes[:, 1], shapes[:, 0]], -1).astype(np.float64)     # (W_l, H_l)
    with np.errstate(invalid="ignore"):
        loc = ref.reshape(bs, nq, 1, 1, 1, 2) + off / norm[None, None, None, :, None, :]
    return loc, attn


def msda_linear(tokens, raw, ref, shapes, query_cam, live=None):
    """tokens [bs, cams, Nv, 256]; raw fp32 [bs, nq, 384]; ref fp32 [bs, nq, 2]; query_cam [nq] (-1: capacity slot) ->
    (row, abs_sum, grad_sum), float64 [bs, nq, 2176]: columns [h * 256, (h + 1) * 256) the sampled sums of the raw token
    channels with head h's locations and weights, column 2048 + h the sum of head h's valid tap weights, the rest 0. Rows of
    capacity slots and rows from `live` on are 0."""
    tokens, shapes, qc = f64(tokens), _i64(shapes), _i64(query_cam)
    bs, cams = tokens.shape[:2]
    nq = qc.shape[0]
    loc, attn = msda_offsets(raw, ref, shapes)
    row, ab, gr = (np.zeros((bs, nq, ROW)) for _ in range(3))
    on = (qc >= 0) & (np.arange(nq) < (nq if live is None else live))
    for cam in range(cams):
        q = np.nonzero(on & (np.minimum(qc, cams - 1) == cam))[0]
        if q.size == 0:
            continue
        value = np.broadcast_to(tokens[:, cam][:, :, None, :], tokens[:, cam].shape[:2] + (HEADS, CH))
        o, a, g, ws = _msda(value, shapes, loc[:, q], attn[:, q])
        row[:, q, :HEADS * CH], ab[:, q, :HEADS * CH], gr[:, q, :HEADS * CH] = (t.reshape(bs, q.size, -1) for t in (o, a, g))
        row[:, q, HEADS * CH:HEADS * CH + HEADS] = ws
        ab[:, q, HEADS * CH:HEADS * CH + HEADS] = ws
    return row, ab, gr


def dfa_points(anchor, learn, fix_scale, proj, image_wh, cam_valid=None):
    """anchor [bs, A, 11]; learn [bs, A, num_learn * 3] raw; fix_scale [num_fix, 3]; proj [bs, cams, 4, 4]; image_wh
    [bs, cams, 2] -> dict: loc [bs, A, P, cams, 2] (a masked camera: -1), depth [bs, A, P, cams] before the clamp, bound
    [bs, A, P, cams, 2] = 8 * 2^-24 * (sum|terms of u| / d + |u| * sum|terms of d| / d^2) / w with the terms expanded
    down to the inputs (the 0.5 of `sigmoid - 0.5` included); where the depth is clamped beyond doubt, d is a constant and
    its term is |u| / d (the rounding of the quotient alone)."""
    an, lr, fs, M, wh = f64(anchor), f64(learn), f64(fix_scale), f64(proj), f64(image_wh)
    bs, A = an.shape[:2]
    size = np.exp(an[:, :, None, 3:6])
    sig = 1.0 / (1.0 + np.exp(-lr.reshape(bs, A, -1, 3)))
    k = np.concatenate([np.broadcast_to(fs[None, None] * size, (bs, A) + fs.shape), (sig - 0.5) * size], 2)
    k_abs = np.concatenate([np.broadcast_to(np.abs(fs)[None, None] * size, (bs, A) + fs.shape), (sig + 0.5) * size], 2)
    sn, cs = an[:, :, None, 6], an[:, :, None, 7]
    p3 = np.stack([cs * k[..., 0] - sn * k[..., 1] + an[:, :, None, 0], sn * k[..., 0] + cs * k[..., 1] + an[:, :, None, 1],
                   k[..., 2] + an[:, :, None, 2]], -1)                                                      # [bs, A, P, 3]
    p3_abs = np.stack([np.abs(cs) * k_abs[..., 0] + np.abs(sn) * k_abs[..., 1] + np.abs(an[:, :, None, 0]),
                       np.abs(sn) * k_abs[..., 0] + np.abs(cs) * k_abs[..., 1] + np.abs(an[:, :, None, 1]),
                       k_abs[..., 2] + np.abs(an[:, :, None, 2])], -1)
    R, t = M[:, None, None, :, :3, :3], M[:, None, None, :, :3, 3]                                          # [bs, 1, 1, cams, 3, (3)]
    uvd = (R * p3[:, :, :, None, None, :]).sum(-1) + t                                                      # [bs, A, P, cams, 3]
    uvd_abs = (np.abs(R) * p3_abs[:, :, :, None, None, :]).sum(-1) + np.abs(t)
    depth = uvd[..., 2]
    d = np.maximum(depth, 1e-5)[..., None]
    w = wh[:, None, None]
    loc = uvd[..., :2] / d / w
    bound = 8 * 2.0 ** -24 * (uvd_abs[..., :2] / d + np.abs(uvd[..., :2]) * uvd_abs[..., 2:3] / d ** 2) / w
    # a depth below the clamp by more than its own fp32 error is the constant 1e-5f in fp32 too: the depth term falls away
    sure = (depth < 1e-5 - 8 * 2.0 ** -24 * uvd_abs[..., 2])[..., None]
    bound = np.where(sure, 8 * 2.0 ** -24 * (uvd_abs[..., :2] / d + np.abs(uvd[..., :2]) / d) / w, bound)
    if cam_valid is not None:
        off = ~np.asarray(f64(cam_valid) != 0)[:, None, None, :]
        loc = np.where(off[..., None], -1.0, loc)
    return dict(loc=loc, depth=depth, bound=bound)


def dfa_weights(feat_logits, cam_logits, L, P, G, cam_valid=None):
    """feat_logits [bs, A, L * P * G]; cam_logits [bs, cams, L * P * G] -> [bs, A, P, cams, L, G]: softmax of their sum over
    cams * L * P per group; a camera with cam_valid[b, cam] = 0 leaves the softmax (weight 0, its logits are not read)."""
    fl, cl = f64(feat_logits), f64(cam_logits)
    bs, A = fl.shape[:2]
    cams = cl.shape[1]
    on = np.ones((bs, cams), bool) if cam_valid is None else np.asarray(f64(cam_valid) != 0)
    cl = np.where(on[:, :, None], cl, 0.0)
    lg = fl.reshape(bs, A, 1, L, P, G) + cl.reshape(bs, 1, cams, L, P, G)
    lg = np.where(on[:, None, :, None, None, None], lg, -np.inf)
    m = lg.max(axis=(2, 3, 4), keepdims=True)
    e = np.where(on[:, None, :, None, None, None], np.exp(lg - m), 0.0)
    w = e / e.sum(axis=(2, 3, 4), keepdims=True)
    return w.transpose(0, 1, 4, 2, 3, 5)


def bound_b(got, want):
    """max |got - want| / (2e-5 * max(1, max |want|))."""
    got, want = f64(got), f64(want)
    return float(np.abs(got - want).max() / (2e-5 * max(1.0, float(np.abs(want).max())))) if want.size else 0.0


TINY = 2.0 ** -126


def kappa_needed(got, want, abs_sum, grad_sum):
    """The smallest kappa that keeps |got - want| under HALF of the bound with twice that kappa on every element:
    |got - want| <= kappa * 2^-24 * abs_sum + (grad_sum + tiny) / 2."""
    got, want = f64(got), f64(want)
    over = np.abs(got - want) - 0.5 * (grad_sum + TINY)
    if ((over > 0) & (abs_sum == 0)).any():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(over > 0, over / (2.0 ** -24 * abs_sum), 0.0)
    return float(k.max()) if k.size else 0.0
