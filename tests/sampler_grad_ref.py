"""The gradients of the two deformable samplers stated in float64, tap by tap (numpy only; nothing of the package under
test is imported). Companion of tests/sampler_ref.py, whose forward statements these differentiate.

  daf_grad     3D deformable aggregation, backward (csrc/deform_agg_bwd.hip)
  msda_grad    camera-grouped multi-scale deformable attention, backward (csrc/msda_bwd.hip)

Locations are the fp32 numbers the kernels are given, widened exactly; pixel = loc * size - 0.5 and everything after it is
float64. One sample on one level, with cell (x0, y0) = floor(pixel), fractions (lx, ly) and the four zero-padded corner
values v00 v01 v10 v11 (row, column), contributes
  val          = (1-ly)(1-lx) v00 + (1-ly) lx v01 + ly (1-lx) v10 + ly lx v11
  d val / d px = (1-ly)(v01 - v00) + ly (v11 - v10)          (times W for the normalised location)
  d val / d py = (1-lx)(v10 - v00) + lx (v11 - v01)          (times H)
  d val / d v  = the four tap weights, at the taps inside the map.

Each function returns, per gradient, a dict of float64 arrays of the gradient's shape:
  want       the gradient
  abs_sum    the same sum with every product replaced by its absolute value
  count      (scatter outputs g_feat / g_value) the number of addends that can reach the element
  shift_sum  how far the element can move when every pixel coordinate moves by eps = 2^-23 * (|loc| * size + 0.5), the
             eps of sampler_ref._pixel: each addend is linear in px and in py inside a cell, so the slopes are exact:
               tap weight        |d/dpx| = its row factor, |d/dpy| = its column factor
               val               |d/dpx| = |d val / d px|, likewise y
               d val / d px      |d/dpy| = |v11 - v10 - v01 + v00|, and none along x; likewise d val / d py
  jump       (g_loc) d/dx of bilinear interpolation is discontinuous where the x pixel is an integer (continuous across
             integers of y), likewise d/dy. A (sample, level, axis) whose float64 pixel lies within eps of an integer is
             AMBIGUOUS: the fp32 pixel may floor into either cell. There `want` holds the midpoint of the derivative in the
             two cells and `jump` half their difference (the channel sum of the level, in absolute value), summed over the
             ambiguous levels of the element. Elements without an ambiguous level have jump == 0.
At an ambiguous sample everything else is continuous, but the neighbouring cell has other taps and other slopes: its taps
count into `count` and `shift_sum` of the scatter output, its slopes into `shift_sum` of the others, and abs_sum of g_loc
takes the larger of the two cells."""
import numpy as np

from tests.sampler_ref import TINY, _i64, _pixel, f64

U24 = 2.0 ** -24


def _f32(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float32)


def _cells(p, e, size):
    """(primary cell, other cell, ambiguous) of pixel coordinates p with eps e on an axis of `size` pixels. The other cell
    is the primary one where the coordinate is not ambiguous. Cells are clipped to [-2, size]: a cell out there has both
    taps outside the map."""
    a = np.floor(p)
    n = np.rint(p)
    amb = np.abs(p - n) <= e
    b = np.where(amb, np.where(a == n, n - 1, n), a)
    return np.clip(a, -2, size).astype(np.int64), np.clip(b, -2, size).astype(np.int64), amb


class _Cell:
    """One candidate cell (cx, cy) per sample of a zero-padded map `fpad` [B, H + 4, W + 4, C] (origin at (2, 2))."""

    def __init__(self, fpad, H, W, bi, cx, cy, px, py):
        lx, ly = np.clip(px - cx, 0.0, 1.0), np.clip(py - cy, 0.0, 1.0)
        self.wx, self.wy = (1.0 - lx, lx), (1.0 - ly, ly)
        self.v, self.ok, self.pix = {}, {}, {}
        for r in (0, 1):
            for c in (0, 1):
                y, x = cy + r, cx + c
                self.v[r, c] = fpad[bi, y + 2, x + 2]
                self.ok[r, c] = (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
                self.pix[r, c] = np.clip(y, 0, H - 1) * W + np.clip(x, 0, W - 1)
        v, wx, wy = self.v, self.wx, self.wy
        col = lambda w: w[:, None]   # noqa: E731
        self.val = sum(col(wy[r] * wx[c]) * v[r, c] for r in (0, 1) for c in (0, 1))
        self.aval = sum(col(wy[r] * wx[c]) * np.abs(v[r, c]) for r in (0, 1) for c in (0, 1))
        self.dx = col(wy[0]) * (v[0, 1] - v[0, 0]) + col(wy[1]) * (v[1, 1] - v[1, 0])
        self.dy = col(wx[0]) * (v[1, 0] - v[0, 0]) + col(wx[1]) * (v[1, 1] - v[0, 1])
        self.adx = col(wy[0]) * (np.abs(v[0, 1]) + np.abs(v[0, 0])) + col(wy[1]) * (np.abs(v[1, 1]) + np.abs(v[1, 0]))
        self.ady = col(wx[0]) * (np.abs(v[1, 0]) + np.abs(v[0, 0])) + col(wx[1]) * (np.abs(v[1, 1]) + np.abs(v[0, 1]))
        self.cross = np.abs(v[1, 1] - v[1, 0] - v[0, 1] + v[0, 0])


def _pad(fmap):
    B, H, W, C = fmap.shape
    out = np.zeros((B, H + 4, W + 4, C))
    out[:, 2:H + 2, 2:W + 2] = fmap
    return out


def _one_level(fmap, bi, px, ex, py, ey, top, go, rows, scatter):
    """n samples on one map. fmap [B, H, W, C]; sample s reads map bi[s] at pixel (px, py) +- (ex, ey); top [n, C] = the
    upstream gradient times the sample's weight, go [n, C] the upstream gradient alone; rows [n] = the row of `scatter`'s
    arrays ([rows, C] each: want, abs_sum, count, shift_sum) that pixel 0 of the sample's map has. Adds the value gradient
    into `scatter`; returns the per-sample weight gradient before its channel reduction (want, abs, shift; [n, C] each)
    and the location gradient per axis in pixels (want, abs, shift, jump; [n] each)."""
    _, H, W, C = fmap.shape
    fpad = _pad(fmap)
    xa, xb, ambx = _cells(px, ex, W)
    ya, yb, amby = _cells(py, ey, H)
    cell = {(0, 0): _Cell(fpad, H, W, bi, xa, ya, px, py), (1, 0): _Cell(fpad, H, W, bi, xb, ya, px, py),
            (0, 1): _Cell(fpad, H, W, bi, xa, yb, px, py), (1, 1): _Cell(fpad, H, W, bi, xb, yb, px, py)}
    live = {(0, 0): np.ones_like(ambx), (1, 0): ambx, (0, 1): amby, (1, 1): ambx & amby}   # the distinct candidate cells
    atop = np.abs(top)
    # ---- the value gradient: a scatter of tap weight * top
    g, ga, gc, gs = scatter
    for key, c in cell.items():
        for r in (0, 1):
            for k in (0, 1):
                on = live[key] & c.ok[r, k]
                if not on.any():
                    continue
                i = np.nonzero(on)[0]
                dst = rows[i] + c.pix[r, k][i]
                if key == (0, 0):
                    w = (c.wy[r] * c.wx[k])[i, None]
                    np.add.at(g, dst, w * top[i])
                    np.add.at(ga, dst, w * atop[i])
                np.add.at(gc, dst, 1.0)
                np.add.at(gs, dst, (ex * c.wy[r] + ey * c.wx[k])[i, None] * atop[i])
    # ---- the weight gradient, per channel
    p = cell[0, 0]
    sx = sum(live[k][:, None] * np.abs(c.dx) for k, c in cell.items())
    sy = sum(live[k][:, None] * np.abs(c.dy) for k, c in cell.items())
    ago = np.abs(go)
    gw = (go * p.val, ago * p.aval, ago * (ex[:, None] * sx + ey[:, None] * sy))
    # ---- the location gradient, per axis
    cr = sum(live[k][:, None] * c.cross for k, c in cell.items())
    gl = []
    for d_a, d_b, a_a, a_b, e_other in ((p.dx, cell[1, 0].dx, p.adx, cell[1, 0].adx, ey), (p.dy, cell[0, 1].dy, p.ady, cell[0, 1].ady, ex)):
        one, two = (top * d_a).sum(1), (top * d_b).sum(1)
        gl.append((0.5 * (one + two), np.maximum((atop * a_a).sum(1), (atop * a_b).sum(1)), e_other * (atop * cr).sum(1),
                   0.5 * np.abs(one - two)))
    return gw, gl


def _out(shape, names):
    return {n: np.zeros(shape) for n in names}


def daf_grad(feat, spatial_shape, scale_start, loc, weights, g_out):
    """feat [bs, N, C]; spatial_shape [cams, L, 2] = (H, W); scale_start [cams, L]; loc fp32 [bs, A, P, cams, 2] = (x, y);
    weights [bs, A, P, cams, L, G]; g_out [bs, A, C] -> dict(g_feat [bs, N, C], g_loc [bs, A, P, cams, 2],
    g_w [bs, A, P, cams, L, G]) of dicts (see the module's docstring). A sample counts only when 0 < x < 1 and 0 < y < 1
    on the fp32 values; g_loc is summed over levels and channels and scaled by W and H."""
    feat, w, go_all = f64(feat), f64(weights), f64(g_out)
    ss, st = _i64(spatial_shape), _i64(scale_start)
    loc32 = _f32(loc)
    bs, N, C = feat.shape
    A, P, cams = loc32.shape[1:4]
    L, G = ss.shape[1], w.shape[-1]
    gd = C // G
    with np.errstate(invalid="ignore"):
        keep = (loc32[..., 0] > 0) & (loc32[..., 0] < 1) & (loc32[..., 1] > 0) & (loc32[..., 1] < 1)
    locd = loc32.astype(np.float64)
    gf = _out((bs * N, C), ("want", "abs_sum", "count", "shift_sum"))
    glo = _out(loc32.shape, ("want", "abs_sum", "shift_sum", "jump"))
    gwo = _out(w.shape, ("want", "abs_sum", "shift_sum"))
    scatter = tuple(gf[k] for k in ("want", "abs_sum", "count", "shift_sum"))
    for cam in range(cams):
        b, a, p = np.nonzero(keep[:, :, :, cam])
        if b.size == 0:
            continue
        x, y = locd[b, a, p, cam, 0], locd[b, a, p, cam, 1]
        go = go_all[b, a]
        for lvl in range(L):
            H, W, start = int(ss[cam, lvl, 0]), int(ss[cam, lvl, 1]), int(st[cam, lvl])
            fmap = feat[:, start:start + H * W].reshape(bs, H, W, C)
            (px, ex), (py, ey) = _pixel(x, W), _pixel(y, H)
            top = go * np.repeat(w[b, a, p, cam, lvl], gd, axis=-1)
            gw, gl = _one_level(fmap, b, px, ex, py, ey, top, go, b * N + start, scatter)
            for name, t in zip(("want", "abs_sum", "shift_sum"), gw):
                gwo[name][b, a, p, cam, lvl] = t.reshape(-1, G, gd).sum(-1)
            for axis, size in ((0, W), (1, H)):
                for name, t in zip(("want", "abs_sum", "shift_sum", "jump"), gl[axis]):
                    glo[name][b, a, p, cam, axis] += size * t
    return dict(g_feat={k: v.reshape(bs, N, C) for k, v in gf.items()}, g_loc=glo, g_w=gwo)


def grid_sample_pixel(loc, size):
    """float64 pixel coordinate and eps of the fp32 route grid_sample takes to it: g = 2 loc - 1, ((g + 1) size - 1) / 2.
    Four roundings: of g (|g| <= 2 |loc| + 1, and it reaches the pixel times size / 2), of g + 1 (2 |loc|, likewise), of
    (g + 1) size (2 |loc| size, halved) and of the last difference (the same + 1, halved): at most
    2^-24 * (size (4 |loc| + 0.5) + 0.5) in all. eps is twice that, 2^-23 * (4 |loc| size + size / 2 + 0.5), as
    sampler_ref._pixel is about twice the two roundings of the kernels' route: the oracle is held under HALF of a bound.
    It is what the fp32 ORACLE is measured with; near loc = 0 it is `size` times the eps the kernels are held to."""
    with np.errstate(invalid="ignore", over="ignore"):
        return loc * size - 0.5, 2.0 ** -23 * (4 * np.abs(loc) * size + size / 2 + 0.5)


def msda_grad(value, shapes, loc, attn, query_cam, g_out, pixel=_pixel):
    """value [bs, cams, Nv, heads, ch]; shapes [(H, W)] * L; loc fp32 [bs, nq, heads, L, P, 2] = (x, y) normalised;
    attn [bs, nq, heads, L, P]; query_cam [nq]; g_out [bs, nq, heads * ch] -> dict(g_value [bs, cams, Nv, heads, ch],
    g_loc, g_attn) of dicts (see the module's docstring). Four taps, each zero outside the map; a pixel that is not finite
    or not inside (-1, size) contributes nothing to any of the three (at -1 and at size themselves the location is
    ambiguous like at any other integer: the cell beyond has no tap inside); query_cam < 0 contributes nothing;
    query_cam >= cams reads the last camera. pixel: the (pixel, eps) rule, sampler_ref._pixel unless the fp32 oracle is
    being measured."""
    value, att, go_all = f64(value), f64(attn), f64(g_out)
    shapes, qc = _i64(shapes), _i64(query_cam)
    loc32 = _f32(loc)
    bs, cams, Nv, heads, ch = value.shape
    nq, _, L, P = loc32.shape[1:5]
    go_all = go_all.reshape(bs, nq, heads, ch)
    locd = loc32.astype(np.float64)
    gv = _out((bs * cams * Nv * heads, ch), ("want", "abs_sum", "count", "shift_sum"))
    glo = _out(loc32.shape, ("want", "abs_sum", "shift_sum", "jump"))
    gao = _out(att.shape, ("want", "abs_sum", "shift_sum"))
    scatter = tuple(gv[k] for k in ("want", "abs_sum", "count", "shift_sum"))
    cam_of = np.minimum(qc, cams - 1)
    start = 0
    for lvl in range(L):
        H, W = int(shapes[lvl][0]), int(shapes[lvl][1])
        (px_all, ex_all), (py_all, ey_all) = pixel(locd[:, :, :, lvl, :, 0], W), pixel(locd[:, :, :, lvl, :, 1], H)
        with np.errstate(invalid="ignore"):
            near = (np.isfinite(px_all) & np.isfinite(py_all) & (px_all > -2) & (px_all < W + 1) & (py_all > -2) & (py_all < H + 1))
        near &= (qc >= 0)[None, :, None, None]
        b, q, h, p = np.nonzero(near)
        if b.size:
            cam = cam_of[q]
            # maps: one per (stream, camera, head)
            fmap = value[:, :, start:start + H * W].reshape(bs, cams, H, W, heads, ch).transpose(0, 1, 4, 2, 3, 5)
            fmap = fmap.reshape(bs * cams * heads, H, W, ch)
            bi = (b * cams + cam) * heads + h
            go = go_all[b, q, h]
            top = go * att[b, q, h, lvl, p][:, None]
            # row of g_value's [bs * cams * Nv * heads, ch] view that pixel i of the map has: (.. * Nv + start + i) * heads + h
            # -> _one_level adds pix to the row, so hand it rows in units of pixels and fold the head in afterwards
            sub = tuple(np.zeros((bs * cams * heads * H * W, ch)) for _ in range(4))
            gw, gl = _one_level(fmap, bi, px_all[b, q, h, p], ex_all[b, q, h, p], py_all[b, q, h, p], ey_all[b, q, h, p], top, go,
                                bi * (H * W), sub)
            for dst, src in zip(scatter, sub):
                dst.reshape(bs, cams, Nv, heads, ch)[:, :, start:start + H * W] += \
                    src.reshape(bs, cams, heads, H * W, ch).transpose(0, 1, 3, 2, 4)
            for name, t in zip(("want", "abs_sum", "shift_sum"), gw):
                gao[name][b, q, h, lvl, p] = t.sum(-1)
            for axis, size in ((0, W), (1, H)):
                for name, t in zip(("want", "abs_sum", "shift_sum", "jump"), gl[axis]):
                    glo[name][b, q, h, lvl, p, axis] = size * t
        start += H * W
    return dict(g_value={k: v.reshape(bs, cams, Nv, heads, ch) for k, v in gv.items()}, g_loc=glo, g_attn=gao)


# ------------------------------------------------------------------------------------------------------------------ bounds
def distance(got, ref):
    """|got - want| beyond the interval [want - jump, want + jump] (jump = 0 where the reference has none)."""
    d = np.abs(f64(got) - ref["want"])
    return np.maximum(d - ref["jump"], 0.0) if "jump" in ref else d


def bound_b(got, ref):
    """max distance / (2e-5 * max(1, max |want|))."""
    want = ref["want"]
    return float(distance(got, ref).max() / (2e-5 * max(1.0, float(np.abs(want).max())))) if want.size else 0.0


def bound_e(got, ref, kappa):
    """max over the elements of distance / ((kappa + count) * 2^-24 * abs_sum + shift_sum + tiny)."""
    if not ref["want"].size:
        return 0.0
    count = ref.get("count", 0.0)
    return float((distance(got, ref) / ((kappa + count) * U24 * ref["abs_sum"] + ref["shift_sum"] + TINY)).max())


def kappa_needed(got, ref):
    """The smallest kappa that keeps `got` under HALF of bound (e) taken with twice that kappa on every element:
    distance <= kappa * 2^-24 * abs_sum + (count * 2^-24 * abs_sum + shift_sum + tiny) / 2."""
    count = ref.get("count", 0.0)
    over = distance(got, ref) - 0.5 * (count * U24 * ref["abs_sum"] + ref["shift_sum"] + TINY)
    if ((over > 0) & (ref["abs_sum"] == 0)).any():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(over > 0, over / (U24 * ref["abs_sum"]), 0.0)
    return float(k.max()) if k.size else 0.0
