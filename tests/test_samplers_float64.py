"""The deformable samplers against their float64 statement (tests/sampler_ref.py) at map and gate edges.

Kernels: daf_fwd_rows / daf_fwd_generic (csrc/deform_agg.hip), daf_fused_rows (csrc/deform_agg_fused.hip, with the arithmetic
of dfa_points_kernel / dfa_weights_kernel of csrc/dfa_prep.hip in its prologue), msda_linear_fwd (csrc/msda_lin.hip) and
msda_grouped_fwd<4|8|0> (csrc/msda.hip), each through its entry in plugin/ops.py.

Locations are placed by hand on every level and axis (`marks`): 0 and 1 (gated out in 3D), their fp32 neighbours inside,
the first / an interior / the last pixel centre, the half-pixel border band where one tap row or column is outside the map,
and the point exactly between two centres; crossed in x and y. Pyramids S1 and S2 are the smallest with a multi-row level and
levels of height or width 1. Tokens are seeded N(0, 1) numbers rounded to f16 values (f16 and f32 token forms read the same
numbers), constant-one maps (the output is the sum of valid tap weights) or one-hot maps (an output names the tap read).

Bounds:
  (b) max |got - want| <= 2e-5 * max(1, max |want|), the project's operator tolerance;
  (e) per output element |got - want| <= KAPPA * 2^-24 * abs_sum + grad_sum + tiny (sampler_ref's two extra sums): an error
      confined to a low-weight group, head or level or to a border row is outside it however small it is against max |want|.
KAPPA is twice what the fp32 oracle (oracle/simpb_ref.py evaluated in float32 on the CPU) needs on the same cases; the
non-GPU test test_fp32_oracle_stays_under_half_of_the_bounds measures it and holds the oracle under half of each bound.

Every output the operators allocate is placed inside a larger sentinel-filled buffer (`guarded`), and the sentinel is checked
after every launch. Each test prints its figures (`FIG ...`) before it asserts."""
import contextlib
import functools
import zlib

import numpy as np
import pytest
import torch

from tests import sampler_ref as S

S1 = [(4, 11), (2, 6), (1, 3), (1, 1)]
S2 = [(3, 5), (5, 3), (1, 4), (4, 1)]

# What the fp32 oracle needs over every GPU case of this module, measured by test_fp32_oracle_stays_under_half_of_the_bounds:
# kappa = 0.81 (the linear 2D sampler on S2, bs 1; 0.37 and 0.10 on two more of its cases; 0.00 on every 3D and grouped 2D
# case, where half of grad_sum alone covers the oracle's error). "Needs" = the smallest kappa that keeps the oracle under
# HALF of bound (e) taken with twice that kappa (sampler_ref.kappa_needed). KAPPA is twice the figure, rounded up.
KAPPA = 1.7

U24 = 2.0 ** -24
F = np.float32


# ------------------------------------------------------------------------------------------------------------ placement
def marks(n):
    """The hand-placed normalised coordinates of an axis of `n` pixels, as fp32 numbers."""
    m = [0.0, 1.0, np.nextafter(F(0), F(1)), np.nextafter(F(1), F(0)),      # gated out; the gate's fp32 neighbours
         0.5 / n, 1 - 0.5 / n,                                               # first / last centre (lh == 0)
         0.25 / n, 1 - 0.25 / n]                                             # border band: one tap row outside
    if n >= 3:
        m.append((n // 2 + 0.5) / n)                                         # an interior centre
    if n >= 2:
        m.append((n // 2) / n)                                               # exactly between two centres
    return [F(v) for v in m]


def numerators(n):
    """`marks(n)` in pixels: offsets whose fp32 quotient by n is the mark (the first centre, the band, ...). Two entries are
    neighbours of the gate values rather than their quotients: 1e-30 stands where marks() has nextafter(0, 1) (a positive
    offset far below any pixel fraction), and nextafter(n, 0) / n rounds to nextafter(1, 0) or to 1."""
    m = [0.0, float(n), 1e-30, float(np.nextafter(F(n), F(0))), 0.5, n - 0.5, 0.25, n - 0.25]
    if n >= 3:
        m.append(n // 2 + 0.5)
    if n >= 2:
        m.append(float(n // 2))
    return [F(v) for v in m]


def cross(pyramids, make=marks):
    """[n, 2] fp32 (x, y): the marks of every width crossed with the marks of every height."""
    xs = sorted({float(v) for p in pyramids for _, w in p for v in make(w)})
    ys = sorted({float(v) for p in pyramids for h, _ in p for v in make(h)})
    return np.array([(x, y) for x in xs for y in ys], dtype=np.float32)


def spread(cr, slots, seed):
    """`slots` rows of `cr`, walking it with a stride coprime to its length: every row is used once slots >= len(cr)."""
    n = len(cr)
    step = next(s for s in (5, 7, 11, 13, 17) if n % s)
    return cr[(np.arange(slots) * step + seed) % n]


def f16_randn(rs, shape):
    return rs.standard_normal(shape).astype(np.float16).astype(np.float32)


def format_maps(groups):
    """feature_maps_format's layout by hand: groups = [[maps [bs, K, C, H, W] per level] per camera set]."""
    cols, ss, st, start = [], [], [], 0
    for maps in groups:
        for cam in range(maps[0].shape[1]):
            ss.append([m.shape[-2:] for m in maps])
            st.append([])
            for m in maps:
                bs, _, c, h, w = m.shape
                cols.append(m[:, cam].reshape(bs, c, h * w).transpose(0, 2, 1))
                st[-1].append(start)
                start += h * w
    return np.ascontiguousarray(np.concatenate(cols, 1)), np.array(ss, np.int32), np.array(st, np.int32)


def make_maps(rs, content, bs, k, c, pyramid):
    out = []
    for h, w in pyramid:
        if content == "random":
            out.append(f16_randn(rs, (bs, k, c, h, w)))
        elif content == "ones":
            out.append(np.ones((bs, k, c, h, w), np.float32))
        else:   # one-hot: a single 1.0 per level, camera and stream
            m = np.zeros((bs, k, c, h * w), np.float32)
            hot = rs.randint(0, h * w, (bs, k))
            for b in range(bs):
                for cam in range(k):
                    m[b, cam, :, hot[b, cam]] = 1.0
            out.append(m.reshape(bs, k, c, h, w))
    return out


# ----------------------------------------------------------------------------------------------------------------- bounds
def figures(got, want, ab, gr):
    """(figure against (b), figure against (e)): 1.0 = on the bound."""
    got, want = S.f64(got), S.f64(want)
    bound = KAPPA * U24 * ab + gr + S.TINY
    return S.bound_b(got, want), float((np.abs(got - want) / bound).max()) if want.size else 0.0


def check(name, got, want, ab, gr):
    assert np.isfinite(S.f64(got)).all(), name
    b, e = figures(got, want, ab, gr)
    print(f"FIG {name} b={b:.3f} e={e:.3f}")
    assert b <= 1.0, (name, "bound (b)", b)
    assert e <= 1.0, (name, "bound (e)", e)


# ------------------------------------------------------------------------------------------------ outputs inside a sentinel
SENTINEL, PAD = -6.02e23, 1024


class _GuardedTorch:
    """Stands in for `torch` inside plugin/ops.py: every output the operators allocate lies inside a sentinel-filled buffer
    (and holds the sentinel itself where torch.empty is asked for)."""

    def __init__(self):
        self.buffers = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, fill, *shape, **kw):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        n = int(np.prod(shape))
        whole = torch.full((n + 2 * PAD,), SENTINEL, dtype=kw.get("dtype") or torch.float32, device=kw["device"])
        inner = whole[PAD:PAD + n].view(shape)
        if fill is not None:
            inner.fill_(fill)
        self.buffers.append((whole, n))
        return inner

    def empty(self, *shape, **kw):
        return self._alloc(None, *shape, **kw)

    def zeros(self, *shape, **kw):
        return self._alloc(0.0, *shape, **kw)

    def holds(self, *tensors):
        """Every tensor an operator returned lies inside one of the guarded buffers."""
        for t in tensors:
            assert any(w.data_ptr() + PAD * w.element_size() <= t.data_ptr() and
                       t.data_ptr() + t.numel() * t.element_size() <= w.data_ptr() + (PAD + n) * w.element_size()
                       for w, n in self.buffers), "an output was allocated outside the guarded buffers"
        self.held = True

    def check(self):
        assert self.buffers and getattr(self, "held", False)
        for whole, n in self.buffers:
            assert bool((whole[:PAD] == SENTINEL).all()) and bool((whole[PAD + n:] == SENTINEL).all()), "write outside the output"


@contextlib.contextmanager
def guarded():
    from simpb_amd.plugin import ops
    real, g = ops.torch, _GuardedTorch()
    ops.torch = g
    try:
        yield g
    finally:
        ops.torch = real
    torch.cuda.synchronize()
    g.check()


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return t.cuda() if dtype is None else t.cuda().to(dtype)


# ============================================================================================ A. drop-in 3D operator
A_SHAPES = dict(
    fast256=dict(C=256, G=8, P=13, K=6, pyr=[S1]),          # daf_fwd_rows, the shipped layout
    fast64=dict(C=64, G=4, P=3, K=2, pyr=[S2]),             # daf_fwd_rows, a partial wave
    generic30=dict(C=30, G=3, P=4, K=3, pyr=[S1]),          # daf_fwd_generic: C % 4 != 0
    generic150=dict(C=256, G=8, P=25, K=6, pyr=[S2]),       # daf_fwd_generic: P * K = 150 > 128
    percam=dict(C=256, G=8, P=13, K=6, pyr=[S1, S2]),       # cameras 0-2 on S1, 3-5 on S2
)
A_RUNS = [(1, 1, "random"), (3, 70, "random"), (1, 70, "ones"), (3, 70, "onehot")]
A_CASES = [(s, *r) for s in A_SHAPES for r in A_RUNS]


@functools.lru_cache(maxsize=None)
def a_case(shape, bs, A, content):
    s = A_SHAPES[shape]
    rs = np.random.RandomState(zlib.crc32(f"{shape} {bs} {A} {content}".encode()))
    per = s["K"] // len(s["pyr"])
    groups = [make_maps(rs, content, bs, per, s["C"], p) for p in s["pyr"]]
    col, ss, st = format_maps(groups)
    cr = cross(s["pyr"])
    loc = spread(cr, bs * A * s["P"] * s["K"], seed=bs + A).reshape(bs, A, s["P"], s["K"], 2)
    w = rs.uniform(0, 1, (bs, A, s["P"], s["K"], len(s["pyr"][0]), s["G"])) * 2.0 ** -np.arange(s["G"])   # low-weight groups
    w = w.astype(np.float32)
    want = S.daf(col, ss, st, loc, w)
    return dict(groups=groups, col=col, ss=ss, st=st, loc=loc, w=w, want=want, full=bs * A * s["P"] * s["K"] >= len(cr))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,bs,A,content", A_CASES)
def test_drop_in_3d_operator(shape, bs, A, content):
    from simpb_amd.plugin import ops
    c = a_case(shape, bs, A, content)
    groups = [[dev(m) for m in maps] for maps in c["groups"]]
    fm = ops.feature_maps_format(groups if len(groups) > 1 else groups[0])
    assert np.array_equal(fm[0].cpu().numpy(), c["col"]) and np.array_equal(fm[1].cpu().numpy(), c["ss"])
    assert np.array_equal(fm[2].cpu().numpy(), c["st"])
    if (bs, A) == (3, 70):
        assert c["full"]            # every crossed mark is sampled
    with guarded() as g:
        out = ops.deformable_aggregation_function(fm[0], fm[1], fm[2], dev(c["loc"]), dev(c["w"]))
        g.holds(out)
    got = out.cpu().numpy()
    check(f"A {shape} bs{bs} A{A} {content}", got, *c["want"])


# =============================================================================================== B. fused 3D kernel
CAMS, LVL, NFIX, NLEARN, NPTS, GRP = 6, 4, 7, 6, 13, 8
LPG = LVL * NPTS * GRP
T_CAM = np.array([(0, 0), (0.125, -0.25), (-0.125, 0.5), (0.25, 0.125), (0, 0), (-0.5, -0.125)], np.float32)
FIX_SCALE = np.array([[0, 0, 0], [0.45, 0, 0], [-0.45, 0, 0], [0, 0.45, 0], [0, -0.45, 0], [0, 0, 0.45], [0, 0, -0.45]], np.float32)
B_CASES = [("exact", "dominant"), ("exact", "equal"), ("affine", "random"), ("scene", "random"), ("scene", "dominant")]
B_MASKED = [("exact", "dominant"), ("affine", "random"), ("scene", "random")]
DROP = np.array([[1] * 6, [1, 0, 1, 1, 0, 1], [1] * 6], np.uint8)       # cameras {1, 4} masked in one stream of three
SCENE_SEED = 3                                                         # chosen on the CPU: see test_scene_seed_...


def b_logits(rs, kind, bs, A):
    if kind == "equal":
        return np.full((bs, A, LPG), 0.7, np.float32), np.full((bs, CAMS, LPG), -0.2, np.float32)
    scale = 2.0 if kind == "random" else 1.0
    fl = (rs.standard_normal((bs, A, LVL * NPTS, GRP)) * scale).astype(np.float32)
    cl = (rs.standard_normal((bs, CAMS, LPG)) * 0.5).astype(np.float32)
    if kind == "dominant":    # one entry per group 30 above the rest
        hot = rs.randint(0, LVL * NPTS, (bs, A, GRP))
        np.put_along_axis(fl, hot[:, :, None, :], 30.0, axis=2)
    return fl.reshape(bs, A, LPG), cl


@functools.lru_cache(maxsize=None)
def b_case(family, logits):
    rs = np.random.RandomState(5 + len(family) + 3 * len(logits))
    bs = 3
    if family == "exact":
        pyr = [S1, S1]
        cr = cross([S1])
        A = -(-len(cr) // bs)
        anchor = np.zeros((bs, A, 11), np.float32)
        anchor[..., 7] = 1.0                                   # yaw (sin, cos) = (0, 1); sizes 0 -> exp = 1
        anchor[..., 2] = rs.standard_normal((bs, A))           # z meets a zero column of the matrix
        target = np.zeros((bs, A), np.int64)
        for i in range(bs * A):
            m = cr[i % len(cr)]
            cam = i % CAMS
            xy = (m.astype(np.float64) - T_CAM[cam]).astype(np.float32)
            if not np.array_equal(xy + T_CAM[cam], m):         # (fp32 sum) the mark is not reachable through this camera's t
                cam, xy = 0, m
            anchor[i % bs, i // bs, :2], target[i % bs, i // bs] = xy, cam
        proj = np.zeros((bs, CAMS, 4, 4), np.float32)
        proj[:, :, 0, 0] = proj[:, :, 1, 1] = proj[:, :, 2, 3] = proj[:, :, 3, 3] = 1.0
        proj[:, :, 0, 3], proj[:, :, 1, 3] = T_CAM[:, 0], T_CAM[:, 1]
        wh = np.ones((bs, CAMS, 2), np.float32)
        fix, learn = np.zeros((NFIX, 3), np.float32), np.zeros((bs, A, NLEARN * 3), np.float32)
        extra = dict(target=target, cross=cr)
    elif family == "affine":      # non-zero fix_scale, learnable offsets and yaw; power-of-two image sizes
        pyr, A = [S1, S2], 48
        anchor = np.zeros((bs, A, 11), np.float32)
        anchor[..., :2] = rs.standard_normal((bs, A, 2)) * 2
        anchor[..., 2] = rs.uniform(2, 10, (bs, A))
        anchor[..., 3:6] = rs.standard_normal((bs, A, 3)) * 0.3
        yaw = rs.uniform(-np.pi, np.pi, (bs, A))
        anchor[..., 6], anchor[..., 7] = np.sin(yaw), np.cos(yaw)
        proj = np.zeros((bs, CAMS, 4, 4), np.float32)
        for cam in range(CAMS):
            f = 28.0 + 2 * cam
            proj[:, cam, :3] = [[f, 0.5, 32.0, 1.0 - cam], [-0.25, f / 2, 16.0, 0.5 * cam], [0.01, -0.02, 1.0, 0.25 * cam]]
        proj[:, :, 3, 3] = 1.0
        wh = np.tile(np.array([64.0, 32.0], np.float32), (bs, CAMS, 1))
        fix = rs.uniform(-0.5, 0.5, (NFIX, 3)).astype(np.float32)
        learn = rs.standard_normal((bs, A, NLEARN * 3)).astype(np.float32)
        extra = {}
    else:                          # the synthetic scene: camera ring, anchors around the ego vehicle
        from simpb_amd import synth
        pyr, A = [S1, S2], 48
        metas = synth.frame_metas(bs, 0)
        proj, wh = metas["projection_mat"].numpy().astype(np.float32), metas["image_wh"].numpy().astype(np.float32)
        anchor = np.stack([synth.anchors(A, seed=SCENE_SEED + b) for b in range(bs)]).astype(np.float32)
        anchor[..., :2] *= 0.5     # more key points inside the images
        fix = FIX_SCALE
        learn = rs.standard_normal((bs, A, NLEARN * 3)).astype(np.float32)
        extra = {}
    groups = [make_maps(rs, "random", bs, 3, 256, p) for p in pyr]
    col, ss, st = format_maps(groups)
    fl, cl = b_logits(rs, logits, bs, A)
    c = dict(col=col, ss=ss, st=st, anchor=anchor, learn=learn, fix=fix, proj=proj, wh=wh, fl=fl, cl=cl, bs=bs, A=A, **extra)
    c["points"] = S.dfa_points(anchor, learn, fix, proj, wh)
    return c


def gate(loc):
    with np.errstate(invalid="ignore"):
        return (loc[..., 0] > 0) & (loc[..., 0] < 1) & (loc[..., 1] > 0) & (loc[..., 1] < 1)


def undecided(points):
    """Samples with a float64 coordinate within the fp32 error bound of 0 or 1: either gate decision is right."""
    loc, bound = points["loc"], points["bound"]
    return ((np.abs(loc) <= bound) | (np.abs(loc - 1) <= bound)).any(-1)


def test_exact_placement_is_exact_and_realises_every_mark():
    """Every operation of the projection is exact in fp32 on the exact-placement input: the float64 locations are fp32
    numbers already or one correctly rounded sum away from one (stage 1 compares bits with float32(reference)); rounding
    never crosses the gate; and the crossed marks all appear, bit for bit, in their target camera."""
    c = b_case("exact", "dominant")
    loc = c["points"]["loc"]
    assert np.array_equal(gate(loc), gate(loc.astype(np.float32)))           # no sample undecided
    assert (c["points"]["depth"] == 1.0).all()
    b, a = np.meshgrid(np.arange(c["bs"]), np.arange(c["A"]), indexing="ij")
    hit = loc[b, a, :, c["target"]]                                          # [bs, A, P, 2]
    assert (hit == hit[:, :, :1]).all()
    seen = {tuple(v) for v in hit[:, :, 0].reshape(-1, 2).astype(np.float32).tolist()}
    assert seen == {tuple(v) for v in c["cross"].tolist()}
    assert (c["target"] != 0).sum() > c["target"].size // 3                    # a camera with t != 0 carries its share


def scene_counts(c):
    p = c["points"]
    und = undecided(p)
    return int(gate(p["loc"]).sum()), int((p["depth"] <= 1e-5).sum()), int(und.sum()), int(und.any(axis=(2, 3)).sum())


def test_scene_seed_leaves_the_gate_decided():
    """The reference alone: >= 200 valid samples, >= 30 samples behind a camera (depth <= 1e-5, the clamp engages), and at
    most 2 % of the anchors carry an undecided sample (they are left out of stage 1's gate comparison)."""
    for logits in ("random", "dominant"):
        c = b_case("scene", logits)
        valid, clamped, und, left = scene_counts(c)
        print(f"FIG scene valid={valid} clamped={clamped} undecided={und} anchors_left_out={left} of {c['bs'] * c['A']}")
        assert valid >= 200 and clamped >= 30 and left <= 0.02 * c["bs"] * c["A"]
    c = b_case("affine", "random")
    valid, _, und, left = scene_counts(c)
    print(f"FIG affine valid={valid} undecided={und} anchors_left_out={left} of {c['bs'] * c['A']}")
    assert valid >= 200 and left <= 0.02 * c["bs"] * c["A"]


def b_reference(c, tokens, loc32, w32, mask):
    """sampler_ref.daf on the kernel's own operands; a masked stream is evaluated with its masked cameras removed."""
    if mask is None or bool(mask.all()):
        return S.daf(tokens, c["ss"], c["st"], loc32, w32)
    parts = []
    for b in range(c["bs"]):
        on = np.nonzero(mask[b])[0]
        parts.append(S.daf(tokens[b:b + 1], c["ss"][on], c["st"][on], loc32[b:b + 1][:, :, :, on], w32[b:b + 1][:, :, :, on]))
    return tuple(np.concatenate(t) for t in zip(*parts))


def run_fused(family, logits, tok, mask_kind):
    from simpb_amd.plugin import ops
    c = b_case(family, logits)
    name = f"B {family} {logits} {tok} {mask_kind}"
    mask = dict(none=None, ones=np.ones((c["bs"], CAMS), np.uint8), drop=DROP)[mask_kind]
    tokens, proj, cl = c["col"].copy(), c["proj"].copy(), c["cl"].copy()
    if mask is not None:      # nothing of a masked camera is read: its tokens, matrix and logits hold NaN
        for b, cam in zip(*np.nonzero(mask == 0)):
            lo, hi = c["st"][cam, 0], c["st"][cam, -1] + c["ss"][cam, -1].prod()
            tokens[b, lo:hi], proj[b, cam], cl[b, cam] = np.nan, np.nan, np.nan
    feat = dev(tokens, torch.float16 if tok == "f16" else torch.float32).contiguous()
    with guarded() as g:
        out, loc, w = ops.dfa_fused(feat, dev(c["ss"]), dev(c["st"]), dev(c["anchor"]), dev(c["learn"]), dev(c["fix"]), dev(proj),
                                    dev(c["wh"]), dev(c["fl"]), dev(cl), GRP, want_operands=True,
                                    cam_valid=dev(mask) if mask is not None else None)
        g.holds(out, loc, w)
    out, loc, w = out.cpu().numpy(), loc.cpu().numpy(), w.cpu().numpy()
    # ---- stage 1: the operands against float64
    pts = c["points"] if mask is None else S.dfa_points(c["anchor"], c["learn"], c["fix"], c["proj"], c["wh"], mask)
    want_w = S.dfa_weights(c["fl"], c["cl"], LVL, NPTS, GRP, mask)
    werr = float(np.abs(w - want_w).max())
    print(f"FIG {name} stage1 weights={werr:.2e}")
    assert werr <= 1e-6, (name, werr)
    off = np.zeros((c["bs"], CAMS), bool) if mask is None else mask == 0
    assert (loc[np.broadcast_to(off[:, None, None, :], loc.shape[:4])] == -1.0).all() and (w[np.broadcast_to(off[:, None, None, :], loc.shape[:4])] == 0.0).all()
    ref = pts["loc"]
    if family == "exact":
        assert np.array_equal(loc, ref.astype(np.float32)), name          # bit equality
        left = 0
    else:
        near = (pts["depth"] > 1e-3) & ~off[:, None, None, :]
        ratio = float((np.abs(loc - ref)[near] / pts["bound"][near]).max())
        und = undecided(pts) & ~off[:, None, None, :]
        keep = ~und.any(axis=(2, 3))                                         # anchors with every sample decided
        left = int((~keep).sum())
        print(f"FIG {name} stage1 loc={ratio:.3f} undecided={int(und.sum())} anchors_left_out={left}")
        assert ratio <= 1.0, (name, ratio)
        assert left <= 0.02 * c["bs"] * c["A"]
        assert np.array_equal(gate(loc)[keep], gate(ref)[keep]), name
    # ---- stage 2: the aggregation on the kernel's own operands (the gate is decided on identical numbers)
    on = np.ones((c["bs"], CAMS), bool) if mask is None else mask != 0
    want = b_reference(c, c["col"], loc, w, on)
    check(name, out, *want)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tok", ["f32", "f16"])
@pytest.mark.parametrize("family,logits", B_CASES)
def test_fused_3d_kernel(family, logits, tok):
    run_fused(family, logits, tok, "none")


@pytest.mark.gpu
@pytest.mark.parametrize("tok", ["f32", "f16"])
@pytest.mark.parametrize("mask_kind", ["ones", "drop"])
@pytest.mark.parametrize("family,logits", B_MASKED)
def test_fused_3d_kernel_with_a_camera_mask(family, logits, tok, mask_kind):
    run_fused(family, logits, tok, mask_kind)


# ============================================================================================ C. linear 2D sampler
NQ, LIVE = 64, 53                                         # 11 capacity slots (query_cam = -1)
M_LIVE = 50                                               # the device-side live count cuts into the last camera group:
                                                          # slots 50-52 carry a camera, `q >= *m_live` alone leaves them out
GROUPS = [(0, 9), (9, 9), (9, 20), (20, 31), (31, 42), (42, 53)]     # six camera groups, one of them empty
FAR = [1e4, -1e4, 3e9, -3e9, np.inf, -np.inf]
C_CASES = [(1, "S1"), (2, "S2"), (2, "S1"), (1, "S2")]
PYR = dict(S1=S1, S2=S2)


def query_cam(groups, nq):
    qc = np.full(nq, -1, np.int32)
    for i, (s, e) in enumerate(groups):
        qc[s:e] = i
    return qc


@functools.lru_cache(maxsize=None)
def c_case(bs, pyr):
    shapes = PYR[pyr]
    rs = np.random.RandomState(31 + bs + len(pyr) + shapes[0][0])
    nv = sum(h * w for h, w in shapes)
    tokens = f16_randn(rs, (bs, CAMS, nv, 256))
    ref = rs.uniform(0, 1, (bs, NQ, 2)).astype(np.float32)
    ref[:, 0::2] = 0.0                                    # even slots: loc = offset / size, the fp32 quotient IS the mark
    off = np.zeros((bs, NQ, S.HEADS, S.LVLS, S.PTS, 2), np.float32)
    slots = bs * NQ * S.HEADS * S.PTS
    for l, (h, w) in enumerate(shapes):
        num = spread(cross([[(h, w)]], numerators), slots, seed=l).reshape(bs, NQ, S.HEADS, S.PTS, 2)
        mark = spread(cross([[(h, w)]]), slots, seed=l).reshape(bs, NQ, S.HEADS, S.PTS, 2).astype(np.float64)
        odd = ((mark - ref[:, :, None, None, :]) * np.array([w, h], np.float64)).astype(np.float32)
        off[:, 0::2, :, l], off[:, 1::2, :, l] = num[:, 0::2], odd[:, 1::2]
    for j, far in enumerate(FAR):                         # one coordinate of every sample of head j of slot j far away
        off[:, j, j, :, :, j % 2] = far
    lg = (rs.standard_normal((bs, NQ, S.HEADS, 16)) * 2).astype(np.float32)
    lg[:, 1::3, :, 5] += 40.0                             # one dominant entry
    lg[:, 2::3] = 0.3                                     # all equal
    raw = np.concatenate([off.reshape(bs, NQ, -1), lg.reshape(bs, NQ, -1)], -1)
    qc = query_cam(GROUPS, NQ)
    want = S.msda_linear(tokens, raw, ref, shapes, qc, LIVE)
    return dict(tokens=tokens, raw=raw, ref=ref, shapes=shapes, qc=qc, want=want)


def tables(shapes):
    ss = torch.tensor(shapes, dtype=torch.long)
    return ss, torch.cat([ss.new_zeros(1), ss.prod(1).cumsum(0)[:-1]])


@functools.lru_cache(maxsize=None)
def projections():
    import torch.nn as nn
    torch.manual_seed(5)
    vp, op = nn.Linear(256, 256), nn.Linear(256, 256)
    with torch.no_grad():
        vp.bias.normal_(0, 0.5)      # a value bias of the size of the projected values: the wsum columns must be right
        op.bias.normal_(0, 0.1)
    return vp, op


@functools.lru_cache(maxsize=None)
def c_chain(bs, pyr):
    """value_proj -> msda -> output_proj in float64 on the live slots."""
    c = c_case(bs, pyr)
    vp, op = projections()
    wv, bv, wo, bo = (S.f64(t) for t in (vp.weight, vp.bias, op.weight, op.bias))
    value = (S.f64(c["tokens"]) @ wv.T + bv).reshape(bs, CAMS, -1, 8, 32)
    loc, attn = S.msda_offsets(c["raw"], c["ref"], c["shapes"])
    want = np.zeros((bs, NQ, 256))
    for cam, (s, e) in enumerate(GROUPS):
        if e > s:
            want[:, s:e] = S._msda(value[:, cam], S._i64(c["shapes"]), loc[:, s:e], attn[:, s:e])[0].reshape(bs, e - s, 256) @ wo.T + bo
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("tok", ["f16", "f32"])
@pytest.mark.parametrize("use_m_live", [True, False], ids=["m_live", "no_m_live"])
@pytest.mark.parametrize("bs,pyr", C_CASES)
def test_linear_2d_sampler(bs, pyr, use_m_live, tok):
    from simpb_amd.plugin import dense, ops
    c = c_case(bs, pyr)
    name = f"C bs{bs} {pyr} {'m_live' if use_m_live else 'no_m_live'} {tok}"
    ss, lsi = tables(c["shapes"])
    n = M_LIVE if use_m_live else LIVE       # rows the launch owes (rows are independent: the reference rows below n are the same)
    m_live = torch.tensor([M_LIVE], dtype=torch.int32, device="cuda") if use_m_live else None
    t = dev(c["tokens"], torch.float16 if tok == "f16" else torch.float32).contiguous()
    with guarded() as g:
        agg = ops.msda_linear(t, ss.cuda(), lsi.cuda(), dev(c["raw"]), dev(c["ref"]), dev(c["qc"]), m_live)
        g.holds(agg)
    got = agg.cpu().numpy()
    want, ab, gr = c["want"]
    live = got[:, :n]
    assert np.isfinite(live).all(), name
    check(name, live[..., :2048], want[:, :n, :2048], ab[:, :n, :2048], gr[:, :n, :2048])
    werr = float(np.abs(live[..., 2048:2056] - want[:, :n, 2048:2056]).max())
    print(f"FIG {name} wsum={werr:.2e}")
    assert werr <= 1e-6, (name, werr)
    for j in range(len(FAR)):                               # every tap of the far head has weight 0
        assert (live[:, j, 2048 + j] == 0.0).all() and (live[:, j, 256 * j:256 * (j + 1)] == 0.0).all(), (name, j)
    assert (live[..., 2056:] == 0.0).all(), name            # pad columns
    assert (c["qc"][:LIVE] >= 0).all() and (c["qc"][LIVE:] < 0).all() and M_LIVE < LIVE
    if use_m_live:
        assert (got[:, n:] == np.float32(SENTINEL)).all(), name      # rows from *m_live on and capacity rows: untouched
    else:
        assert (got[:, n:] == 0.0).all(), name
    if bs == 1 or not use_m_live:      # (dense.linear's m_live counts rows of the flat [bs * slots] operand, msda_linear's counts
        vp, op = projections()         # slots of every stream: with bs > 1 the two disagree, and the head passes none there)
        wf, bf = dense.fold_msda_linear(vp.cuda(), op.cuda(), 8, ops.MSDA_LINEAR_WIDTH)
        out = dense.linear(agg, wf, bf, m_live=m_live)[:, :n].cpu().numpy()
        fold = S.bound_b(out, c_chain(bs, pyr)[:, :n])
        print(f"FIG {name} folded b={fold:.3f}")
        assert fold <= 1.0, (name, fold)


# =========================================================================================== D. grouped 2D sampler
D_CASES = [dict(pts=4, heads=8, ch=32, pyr="S1", bs=2), dict(pts=8, heads=16, ch=32, pyr="S2", bs=1),
           dict(pts=3, heads=4, ch=8, pyr="S1", bs=1)]
D_NQ = 40
D_GROUPS = [(0, 8), (8, 8), (8, 15), (16, 24), (24, 30), (30, 35)]      # slot 15 and slots 35-39: capacity (query_cam = -1)


@functools.lru_cache(maxsize=None)
def d_case(i):
    d = D_CASES[i]
    shapes, bs, heads, ch, pts = PYR[d["pyr"]], d["bs"], d["heads"], d["ch"], d["pts"]
    rs = np.random.RandomState(41 + i)
    nv = sum(h * w for h, w in shapes)
    value = f16_randn(rs, (bs, CAMS, nv, heads, ch))
    loc = np.zeros((bs, D_NQ, heads, len(shapes), pts, 2), np.float32)
    for l, (h, w) in enumerate(shapes):
        loc[:, :, :, l] = spread(cross([[(h, w)]]), bs * D_NQ * heads * pts, seed=l).reshape(bs, D_NQ, heads, pts, 2)
    for j, far in enumerate(FAR):
        loc[:, j, j % heads, :, :, j % 2] = far
    attn = (rs.uniform(0, 1, (bs, D_NQ, heads, len(shapes), pts)) * 2.0 ** -(np.arange(heads) % 5)[:, None, None]).astype(np.float32)
    qc = query_cam(D_GROUPS, D_NQ)
    want = [np.zeros((bs, D_NQ, heads * ch)) for _ in range(3)]
    for cam, (s, e) in enumerate(D_GROUPS):
        if e > s:
            for dst, src in zip(want, S.msda(value[:, cam], shapes, loc[:, s:e], attn[:, s:e])):
                dst[:, s:e] = src
    return dict(value=value, loc=loc, attn=attn, qc=qc, shapes=shapes, want=want)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(D_CASES)), ids=["pts4_256", "pts8_512", "pts3_32"])
def test_grouped_2d_sampler(i):
    from simpb_amd.plugin import ops
    c = d_case(i)
    ss, lsi = tables(c["shapes"])
    with guarded() as g:
        out = ops.ms_deform_attn_grouped(dev(c["value"]), ss.cuda(), lsi.cuda(), dev(c["loc"]), dev(c["attn"]), dev(c["qc"]))
        g.holds(out)
    got = out.cpu().numpy()
    assert (got[:, c["qc"] < 0] == 0.0).all()                 # capacity slots give zeros
    heads, ch = D_CASES[i]["heads"], D_CASES[i]["ch"]
    for j in range(len(FAR)):
        assert (got[:, j, (j % heads) * ch:(j % heads + 1) * ch] == 0.0).all(), j
    check(f"D {D_CASES[i]}", got, *c["want"])


# ==================================================================================== CPU: the reference tied to what is pinned
def _R():
    from oracle import simpb_ref
    return simpb_ref


def t32(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def test_nested_feature_maps_format_addresses_every_camera_set():
    """Camera sets with pyramids of their own: the start of every (camera, level) addresses that camera's own rows of the
    concatenated token buffer."""
    from simpb_amd.plugin import ops
    c = a_case("percam", 1, 1, "random")
    col, ss, st = ops.feature_maps_format([[t32(m) for m in maps] for maps in c["groups"]])
    assert np.array_equal(col.numpy(), c["col"]) and np.array_equal(ss.numpy(), c["ss"]) and np.array_equal(st.numpy(), c["st"])
    for cam in range(6):
        for lvl, m in enumerate(c["groups"][cam // 3]):
            h, w = m.shape[-2:]
            rows = col[0, int(st[cam, lvl]):int(st[cam, lvl]) + h * w].numpy()
            assert np.array_equal(rows, m[0, cam % 3].reshape(-1, h * w).T)


def oracle_daf(col, ss, st, loc, w):
    return _R().deformable_aggregation(t32(col), t32(ss), t32(st), t32(loc), t32(w)).numpy()


def test_daf_against_the_oracle_the_c_restatement_and_the_golden_vector():
    from oracle import build_c
    from tests.helpers import load_golden
    from tests.test_oracle_golden import daf_case
    for shape in ("generic30", "percam"):
        c = a_case(shape, 3, 70, "random")
        want = c["want"][0]
        assert S.bound_b(oracle_daf(c["col"], c["ss"], c["st"], c["loc"], c["w"]), want) <= 0.5
        assert S.bound_b(build_c.daf_forward(c["col"], c["ss"], c["st"], c["loc"], c["w"]), want) <= 0.5
    g = load_golden("ops.npz")
    col, ss, ssi, loc, w = daf_case(g)
    out = S.daf(col, ss, ssi, loc, w)[0]
    assert np.abs(out - g["daf.out_fallback"]).max() < 1e-5


def test_msda_against_grid_sample_and_the_oracle():
    import torch.nn.functional as F_
    c = d_case(0)
    shapes, value, loc, attn = c["shapes"], c["value"][:, 0], c["loc"][:, 6:], c["attn"][:, 6:]    # (slots 0-5 hold non-finite locations)
    got = S.msda(value, shapes, loc, attn)[0]
    bs, _, heads, hd = value.shape
    nq, pts = loc.shape[1], loc.shape[4]
    want, start = np.zeros_like(got).reshape(bs, nq, heads, hd), 0
    for l, (h, w) in enumerate(shapes):        # grid_sample in float64, level by level
        v = torch.from_numpy(value[:, start:start + h * w].astype(np.float64)).permute(0, 2, 3, 1).reshape(bs * heads, hd, h, w)
        g = torch.from_numpy(2 * loc[:, :, :, l].astype(np.float64) - 1).permute(0, 2, 1, 3, 4).reshape(bs * heads, nq, pts, 2)
        s = F_.grid_sample(v, g, mode="bilinear", padding_mode="zeros", align_corners=False)            # [bs*heads, hd, nq, pts]
        a = torch.from_numpy(attn[:, :, :, l].astype(np.float64)).permute(0, 2, 1, 3).reshape(bs * heads, 1, nq, pts)
        want += (s * a).sum(-1).reshape(bs, heads, hd, nq).permute(0, 3, 1, 2).numpy()
        start += h * w
    assert np.abs(got - want.reshape(got.shape)).max() <= 1e-12 * max(1.0, np.abs(want).max())
    ora = _R().ms_deform_attn(torch.from_numpy(value).double(), torch.tensor(shapes), torch.from_numpy(loc).double(),
                              torch.from_numpy(attn).double()).numpy()
    assert np.abs(got - ora).max() <= 1e-12 * max(1.0, np.abs(ora).max())


def test_dfa_points_and_weights_against_the_oracle():
    R = _R()
    c = b_case("scene", "random")
    rs = np.random.RandomState(9)
    bs, A = c["bs"], c["A"]
    feature, embed = (torch.from_numpy(rs.standard_normal((bs, A, 256))) for _ in range(2))
    p = {"k.fix_scale": torch.from_numpy(c["fix"]).double(), "k.learnable_fc.weight": torch.from_numpy(rs.standard_normal((18, 256)) * 0.1),
         "k.learnable_fc.bias": torch.from_numpy(rs.standard_normal(18) * 0.1)}
    anchor, proj, wh = (torch.from_numpy(c[k]).double() for k in ("anchor", "proj", "wh"))
    learn = R.linear(p, "k.learnable_fc", feature)
    kp = R.key_points(p, "k", anchor, feature)
    want = R.project_points(kp, proj, wh).permute(0, 2, 3, 1, 4).numpy()
    got = S.dfa_points(c["anchor"], learn.numpy(), c["fix"], c["proj"], c["wh"])
    assert (got["depth"] <= 1e-5).sum() >= 30
    assert np.abs(got["loc"] - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    # weights: weights_fc(feature + embed + camera) = weights_fc(feature + embed) + camera . W^T (no second bias)
    p.update({"m.weights_fc.weight": torch.from_numpy(rs.standard_normal((LPG, 256)) * 0.1), "m.weights_fc.bias": torch.from_numpy(rs.standard_normal(LPG) * 0.1)})
    for i, (k, n) in enumerate((("0", (256, 12)), ("3", (256, 256)))):
        p[f"m.camera_encoder.{k}.weight"] = torch.from_numpy(rs.standard_normal(n) * 0.1)
        p[f"m.camera_encoder.{k}.bias"] = torch.from_numpy(rs.standard_normal(256) * 0.1)
    for k in ("2", "5"):
        p[f"m.camera_encoder.{k}.weight"], p[f"m.camera_encoder.{k}.bias"] = torch.ones(256).double(), torch.zeros(256).double()
    want_w = R.dfa_weights(p, "m", feature, embed, proj).permute(0, 1, 4, 2, 3, 5).numpy()
    cam, _ = R.linear_relu_ln(p, "m.camera_encoder", proj[:, :, :3].reshape(bs, CAMS, -1), 1, 2)
    fl = R.linear(p, "m.weights_fc", feature + embed).numpy()
    cl = (cam @ p["m.weights_fc.weight"].t()).numpy()
    got_w = S.dfa_weights(fl, cl, LVL, NPTS, GRP)
    assert np.abs(got_w - want_w).max() <= 1e-12
    mask = np.array([[1, 0, 1, 1, 0, 1]] * bs, np.uint8)       # masked cameras leave the softmax: the oracle on the four others
    on = np.nonzero(mask[0])[0]
    sub = S.dfa_weights(fl, cl[:, on], LVL, NPTS, GRP)
    got_m = S.dfa_weights(fl, cl, LVL, NPTS, GRP, mask)
    assert np.abs(got_m[:, :, :, on] - sub).max() <= 1e-15 and (got_m[:, :, :, [1, 4]] == 0).all()


def oracle_row(c):
    """The 2176-wide row from the oracle's sampler in float32: softmax, ref + offset / size, ms_deform_attn on the raw token
    channels per head, and on a map of ones for the tap-weight sums."""
    R = _R()
    bs = c["tokens"].shape[0]
    raw, ref, tokens = t32(c["raw"]), t32(c["ref"]), t32(c["tokens"])
    ss = torch.tensor(c["shapes"])
    off = raw[..., :256].view(bs, NQ, 8, 4, 4, 2)
    aw = raw[..., 256:].view(bs, NQ, 8, 16).softmax(-1).view(bs, NQ, 8, 4, 4)
    norm = torch.stack([ss[:, 1], ss[:, 0]], -1).float()
    loc = ref[:, :, None, None, None, :] + off / norm[None, None, None, :, None, :]
    row = torch.zeros(bs, NQ, S.ROW)
    for cam, (s, e) in enumerate(GROUPS):
        if e > s:
            value = tokens[:, cam][:, :, None, :].expand(-1, -1, 8, -1).contiguous()
            row[:, s:e, :2048] = R.ms_deform_attn(value, ss, loc[:, s:e].contiguous(), aw[:, s:e].contiguous())
            row[:, s:e, 2048:2056] = R.ms_deform_attn(torch.ones(bs, value.shape[1], 8, 1), ss, loc[:, s:e].contiguous(), aw[:, s:e].contiguous())
    return row.numpy()


def test_fp32_oracle_stays_under_half_of_the_bounds():
    """The fp32 oracle on every GPU case of this module: its figure against (b) and the kappa it needs for (e). KAPPA is
    twice the largest; the oracle stays under half of each bound. Rows with non-finite locations are left out for the 2D
    oracle (grid_sample gives NaN there; the kernels and the float64 statement give zeros)."""
    R = _R()
    worst_b, worst_k = 0.0, 0.0

    def note(name, got, want, ab, gr):
        nonlocal worst_b, worst_k
        b, k = S.bound_b(got, want), S.kappa_needed(got, want, ab, gr)
        print(f"FIG oracle {name} b={b:.3f} e={figures(got, want, ab, gr)[1]:.3f} kappa={k:.2f}")
        worst_b, worst_k = max(worst_b, b), max(worst_k, k)

    for shape, bs, A, content in A_CASES:
        c = a_case(shape, bs, A, content)
        note(f"A {shape} bs{bs} A{A} {content}", oracle_daf(c["col"], c["ss"], c["st"], c["loc"], c["w"]), *c["want"])
    for family, logits in B_CASES:         # the aggregation stage on the float64 operands rounded to fp32
        c = b_case(family, logits)
        loc = c["points"]["loc"].astype(np.float32)
        w = S.dfa_weights(c["fl"], c["cl"], LVL, NPTS, GRP).astype(np.float32)
        note(f"B {family} {logits}", oracle_daf(c["col"], c["ss"], c["st"], loc, w), *S.daf(c["col"], c["ss"], c["st"], loc, w))
    for bs, pyr in C_CASES:
        c = c_case(bs, pyr)
        got, (want, ab, gr) = oracle_row(c), c["want"]
        q = np.arange(len(FAR), LIVE)
        note(f"C bs{bs} {pyr}", got[:, q, :2048], want[:, q, :2048], ab[:, q, :2048], gr[:, q, :2048])
        assert np.abs(got[:, q, 2048:2056] - want[:, q, 2048:2056]).max() <= 0.5e-6
    for i, d in enumerate(D_CASES):
        c = d_case(i)
        q = np.array([k for k in range(len(FAR), D_NQ) if c["qc"][k] >= 0])
        got = np.zeros_like(c["want"][0])
        for cam, (s, e) in enumerate(D_GROUPS):
            if e > s:
                got[:, s:e] = R.ms_deform_attn(t32(c["value"][:, cam]), torch.tensor(c["shapes"]), t32(c["loc"][:, s:e]), t32(c["attn"][:, s:e])).numpy()
        note(f"D {d}", got[:, q], *(t[:, q] for t in c["want"]))
    print(f"FIG oracle worst b={worst_b:.3f} kappa={worst_k:.2f} KAPPA={KAPPA}")
    assert worst_b <= 0.5
    assert 2 * worst_k <= KAPPA, (worst_k, KAPPA)      # under half of bound (e)
