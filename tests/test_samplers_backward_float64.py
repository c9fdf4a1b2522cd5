"""The two sampler backward kernels against their float64 statement (tests/sampler_grad_ref.py) at map and gate edges.

Kernels: daf_bwd_rows (csrc/deform_agg_bwd.hip) and msda_grouped_bwd (csrc/msda_bwd.hip), each through autograd of its
operator in plugin/ops.py and directly through the C entry point with outputs pre-filled with NaN inside sentinel-padded
buffers.

Locations: half of the samples of every case are the hand-placed marks of test_samplers_float64 (0 and 1, their fp32
neighbours, first / interior / last centre, the border band, between two centres; in 2D also outside [0, 1], on -1 and on
`size` themselves, far away, infinite and NaN), the other half seeded locations at least 1e-3 pixel from every integer on
every level: at a pixel centre d/dx has two one-sided values (`jump`), and test_sampler_grad_ref_host.py holds every case to
at least half of its g_loc elements without one.

Bounds, per gradient:
  (b) max distance <= 2e-5 * max(1, max |want|), the project's operator tolerance;
  (e) per element distance <= (KAPPA_BWD + count) * 2^-24 * abs_sum + shift_sum + tiny,
with distance = |got - want| beyond [want - jump, want + jump]. KAPPA_BWD is twice what the fp32 oracle's autograd needs on
the same cases (tests/test_sampler_grad_ref_host.py::test_fp32_oracle_stays_under_half_of_the_bounds measures it on the CPU).
Each test prints its figures (`FIG ...`) before it asserts."""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

from tests import sampler_grad_ref as G
from tests import sampler_ref as S
from tests.test_samplers_float64 import PAD, S1, S2, SENTINEL, cross, dev, format_maps, guarded, make_maps, marks, spread

# What the fp32 oracle's autograd needs over every case of this module, measured on the CPU by
# test_sampler_grad_ref_host.py::test_fp32_oracle_stays_under_half_of_the_bounds: kappa = 2.19 (g_loc of the 2D case
# 8 heads x 32, L 5, P 8; 2.09 and 2.04 for g_attn on constant maps, 1.75 for g_w of the 3D case pk65 on constant maps; its
# worst figure against (b) is 0.035). "Needs" = the smallest kappa that keeps the oracle under HALF of bound (e) taken with
# twice that kappa (sampler_grad_ref.kappa_needed); the 2D oracle is measured with the eps of grid_sample's own route to the
# pixel (sampler_grad_ref.grid_sample_pixel), the kernels are held to sampler_ref._pixel's. KAPPA_BWD is twice the figure,
# rounded up.
KAPPA_BWD = 4.4

F = np.float32
NONFINITE = [(np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, -np.inf), (np.nan, np.nan), (-np.inf, np.inf)]


def low_block(rs, shape):
    """N(0, 1) upstream gradient with channels [32, 64) scaled by 2^-10."""
    g = rs.standard_normal(shape).astype(F)
    g[..., 32:64] *= F(2.0 ** -10)
    return g


def interior(rs, n, widths, heights, lo, hi, grid=None):
    """n seeded fp32 (x, y) in (lo, hi) whose pixel is at least 1e-3 from every integer on every listed size (grid: multiples
    of 1 / grid only)."""
    def axis(sizes):
        out = []
        while len(out) < n:
            v = F(rs.uniform(lo, hi))
            if grid:
                v = F(np.floor(v * grid) / grid)
            px = np.float64(v) * np.array(sizes, np.float64) - 0.5
            if (np.abs(px - np.rint(px)) >= 1e-3).all():
                out.append(v)
        return np.array(out, F)
    return np.stack([axis(sorted(set(widths))), axis(sorted(set(heights)))], -1)


def interleave(inner, marked):
    """Even slots seeded, odd slots hand-placed."""
    out = np.empty((len(inner) + len(marked), 2), F)
    out[0::2], out[1::2] = inner, marked
    return out


def bits_zero(x):
    return np.ascontiguousarray(x, dtype=F).view(np.int32) == 0


def same_bits(a, b):
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def check(name, got, ref):
    got = S.f64(got)
    assert np.isfinite(got).all(), (name, "not finite", int((~np.isfinite(got)).sum()))
    b, e = G.bound_b(got, ref), G.bound_e(got, ref, KAPPA_BWD)
    print(f"FIG {name} b={b:.3f} e={e:.3f}")
    assert b <= 1.0, (name, "bound (b)", b)
    assert e <= 1.0, (name, "bound (e)", e)


class Padded:
    """A float32 device buffer of n elements pre-filled with NaN inside sentinel padding."""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.whole = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.inner = self.whole[PAD:PAD + self.n]
        self.inner.fill_(float("nan"))
        self.shape = tuple(shape)

    def ptr(self):
        return ctypes.c_void_p(self.inner.data_ptr())

    def result(self, name):
        assert bool((self.whole[:PAD] == SENTINEL).all()) and bool((self.whole[PAD + self.n:] == SENTINEL).all()), (name, "write outside the output")
        assert not bool(torch.isnan(self.inner).any()), (name, "an element was left unwritten")
        return self.inner.view(self.shape)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ================================================================================================= 3D: daf_bwd_rows
S12 = S1 + S2
T_SHAPES = dict(
    shipped=dict(C=256, G=8, P=13, K=6, pyr=[S1]),           # 78 samples: the second ballot word in use
    c64_g1=dict(C=64, G=1, P=3, K=2, pyr=[S2]),              # one channel slot per lane
    c64_g2=dict(C=64, G=2, P=3, K=2, pyr=[S1]),
    c192_g2=dict(C=192, G=2, P=4, K=3, pyr=[S1]),            # the group edge at 96 falls on a half-wave, not a wave
    c192_g3=dict(C=192, G=3, P=4, K=3, pyr=[S2]),
    c192_g6=dict(C=192, G=6, P=4, K=3, pyr=[S1]),
    wide_g1=dict(C=256, G=1, P=2, K=2, pyr=[S2]),            # a group spans several channel slots
    wide_g2=dict(C=256, G=2, P=2, K=2, pyr=[S1]),
    pk1=dict(C=128, G=4, P=1, K=1, pyr=[S1]),
    pk64=dict(C=128, G=4, P=8, K=8, pyr=[S2]),               # the first 64-bit mask full
    pk65=dict(C=128, G=4, P=5, K=13, pyr=[S1]),              # one sample in the second
    pk128=dict(C=128, G=4, P=16, K=8, pyr=[S2]),             # the limit
    lvl1=dict(C=128, G=4, P=3, K=2, pyr=[S1[:1]]),           # three idle waves
    lvl2=dict(C=128, G=4, P=3, K=2, pyr=[S1[:2]]),
    lvl5=dict(C=128, G=4, P=3, K=2, pyr=[S12[:5]]),          # wave 0 walks two levels
    lvl8=dict(C=128, G=4, P=3, K=2, pyr=[S12]),              # every wave walks two
    percam=dict(C=256, G=8, P=13, K=6, pyr=[S1, S2]),        # cameras 0-2 on S1, 3-5 on S2
)
T_RUNS = [(1, 1, "random"), (2, 7, "random"), (1, 7, "ones"), (2, 7, "onehot")]
T_CASES = [(s, *r) for s in T_SHAPES for r in T_RUNS] + [("c64_g2", 1, 7, "gated")]
GATED = np.array([(0, 0.5), (0.5, 1), (1, 1), (-0.5, 0.5), (0.5, 1.5), (np.nan, 0.5), (0.5, np.inf), (0, 0)], F)


@functools.lru_cache(maxsize=None)
def t_case(shape, bs, A, content):
    """Inputs and float64 gradients of one 3D case. content "gated": random maps, every sample of every row gated out."""
    s = T_SHAPES[shape]
    rs = np.random.RandomState(zlib.crc32(f"bwd {shape} {bs} {A} {content}".encode()))
    C, Gr, P, K = s["C"], s["G"], s["P"], s["K"]
    per = K // len(s["pyr"])
    groups = [make_maps(rs, "random" if content == "gated" else content, bs, per, C, p) for p in s["pyr"]]
    col, ss, st = format_maps(groups)
    slots = bs * A * P * K
    if content == "gated":
        loc = GATED[np.arange(slots) % len(GATED)]
    else:
        widths, heights = [w for p in s["pyr"] for _, w in p], [h for p in s["pyr"] for h, _ in p]
        marked = spread(cross(s["pyr"]), slots // 2, seed=bs + A).copy()
        if len(marked) >= 2 * len(NONFINITE):
            marked[:len(NONFINITE)] = NONFINITE
        loc = interleave(interior(rs, slots - slots // 2, widths, heights, 0.01, 0.99), marked)
    loc = loc.reshape(bs, A, P, K, 2).copy()
    if A > 1:
        loc[:, 1] = loc[:, 0]                  # two anchors of every stream aim at the same pixels: the atomics collide
    L = len(s["pyr"][0])
    w = (rs.uniform(0, 1, (bs, A, P, K, L, Gr)) * 2.0 ** -np.arange(Gr)).astype(F)      # low-weight groups
    gout = low_block(rs, (bs, A, C))
    return dict(col=col, ss=ss, st=st, loc=loc, w=w, gout=gout, want=G.daf_grad(col, ss, st, loc, w, gout),
                dims=(bs, K, col.shape[1], C, L, A, P, Gr))


def gate(loc):
    with np.errstate(invalid="ignore"):
        return (loc[..., 0] > 0) & (loc[..., 0] < 1) & (loc[..., 1] > 0) & (loc[..., 1] < 1)


def daf_autograd(col, ss, st, loc, w, gout, need=(True, True, True), transform=None):
    from simpb_amd.plugin import ops
    f, l, wt = (dev(t).requires_grad_(n) for t, n in zip((col, loc, w), need))
    with guarded() as g:
        out = ops.deformable_aggregation_function(f, dev(ss), dev(st), l, wt if transform is None else transform(wt))
        g.holds(out)
    if gout is None:
        out.sum().backward()
    else:
        out.backward(gout)
    torch.cuda.synchronize()
    return f.grad, l.grad, wt.grad


def daf_direct(c):
    from simpb_amd import _lib
    bs, K, N, C, L, A, P, Gr = c["dims"]
    gf, gl, gw = Padded((bs, N, C)), Padded(c["loc"].shape), Padded(c["w"].shape)
    keep = [dev(c[k]) for k in ("col", "ss", "st", "loc", "w", "gout")]
    status = _lib.lib().simpb_deformable_aggregation_backward(gf.ptr(), gl.ptr(), gw.ptr(), *(ptr(t) for t in keep), bs, K, N, C, L, A,
                                                              P, Gr, stream())
    torch.cuda.synchronize()
    assert status == 0, status
    return gf.result("g_feat"), gl.result("g_loc"), gw.result("g_w")


def daf_asserts(name, c, gf, gl, gw):
    want = c["want"]
    gf, gl, gw = gf.cpu().numpy(), gl.cpu().numpy(), gw.cpu().numpy()
    for tag, got in (("g_feat", gf), ("g_loc", gl), ("g_w", gw)):
        check(f"{name} {tag}", got, want[tag])
    off = ~gate(c["loc"])
    assert bits_zero(gl[off]).all() and bits_zero(gw[off]).all(), (name, "a gated sample has a gradient")
    assert bits_zero(gf[want["g_feat"]["count"] == 0]).all(), (name, "a token no sample touches has a gradient")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,bs,A,content", T_CASES)
def test_3d_backward(shape, bs, A, content):
    c = t_case(shape, bs, A, content)
    name = f"3D {shape} bs{bs} A{A} {content}"
    if content == "gated":
        assert not gate(c["loc"]).any()
    auto = daf_autograd(c["col"], c["ss"], c["st"], c["loc"], c["w"], dev(c["gout"]))
    daf_asserts(name + " autograd", c, *auto)
    direct = daf_direct(c)
    daf_asserts(name + " direct", c, *direct)
    # plain stores in a fixed order: the second launch repeats the first bit for bit
    assert same_bits(auto[1], direct[1]) and same_bits(auto[2], direct[2]), (name, "g_loc / g_w differ between two launches")


# ------------------------------------------------------------------------------------- one contribution per element
ONE_LOC = (0.3125, 0.6875)     # on a 4 x 11 map: pixel (2.9375, 2.25), every tap weight a product of two 4-bit fractions


@functools.lru_cache(maxsize=None)
def t_single(content):
    rs = np.random.RandomState(7 + len(content))
    groups = [make_maps(rs, content, 1, 1, 128, [(4, 11)])]
    col, ss, st = format_maps(groups)
    loc = np.array(ONE_LOC, F).reshape(1, 1, 1, 1, 2)
    w = np.array([1.5, 0.75, 0.375, 3.0], F).reshape(1, 1, 1, 1, 1, 4)
    gout = low_block(rs, (1, 1, 128))
    return dict(col=col, ss=ss, st=st, loc=loc, w=w, gout=gout, want=G.daf_grad(col, ss, st, loc, w, gout),
                dims=(1, 1, col.shape[1], 128, 1, 1, 1, 4))


def ulps(got, want):
    """|got - float32(want)| in units of the spacing of float32(want)."""
    w32 = np.asarray(want, np.float64).astype(F)
    return float((np.abs(got.astype(np.float64) - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["random", "onehot"])
def test_3d_backward_single_contribution(content):
    """A = P = K = L = 1: four taps, one addend each, no atomic collision. The tap weights and the group weights have few
    bits, so float32(g_out * weight) * tap weight is one rounding from float64: within 2 ulp."""
    c = t_single(content)
    gf, gl, gw = daf_direct(c)
    daf_asserts(f"3D single {content}", c, gf, gl, gw)
    assert (c["want"]["g_feat"]["count"] <= 1).all() and (c["want"]["g_feat"]["count"] == 1).sum() == 4 * 128
    u = ulps(gf.cpu().numpy(), c["want"]["g_feat"]["want"])
    print(f"FIG 3D single {content} g_feat ulp={u:.2f}")
    assert u <= 2.0, u


# ------------------------------------------------------------------------------------------------- wrapper behaviour
def t_wrapper_case():
    return t_case("c64_g2", 1, 7, "random")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sum", "fp16", "loc_only", "strided_weights"])
def test_3d_wrapper(kind):
    """out.sum().backward() (an expanded, stride-0 upstream gradient), an fp16 upstream gradient, only sampling_location
    requiring grad, and a non-contiguous weights view: the gradients of the plain call, within (e)."""
    c = t_wrapper_case()
    col, ss, st, loc, w = (c[k] for k in ("col", "ss", "st", "loc", "w"))
    name = f"3D wrapper {kind}"
    if kind == "sum":
        want = G.daf_grad(col, ss, st, loc, w, np.ones_like(c["gout"]))
        got = daf_autograd(col, ss, st, loc, w, None)
    elif kind == "fp16":
        g16 = c["gout"].astype(np.float16)
        want = G.daf_grad(col, ss, st, loc, w, g16.astype(F))
        got = daf_autograd(col, ss, st, loc, w, dev(g16))
    elif kind == "loc_only":
        want = c["want"]
        got = daf_autograd(col, ss, st, loc, w, dev(c["gout"]), need=(False, True, False))
        assert got[0] is None and got[2] is None
    else:
        want = c["want"]
        wide = np.zeros(w.shape[:-1] + (2 * w.shape[-1],), F)
        wide[..., ::2] = w
        got = daf_autograd(col, ss, st, loc, wide, dev(c["gout"]), transform=lambda t: t[..., ::2])
        assert bits_zero(got[2][..., 1::2].cpu().numpy()).all()
        got = (got[0], got[1], got[2][..., ::2])
    for tag, g in zip(("g_feat", "g_loc", "g_w"), got):
        if g is not None:
            check(f"{name} {tag}", g.cpu().numpy(), want[tag])


@pytest.mark.gpu
def test_3d_backward_refuses_what_only_the_generic_forward_takes():
    """C = 30: daf_fwd_generic serves the forward, the backward's entry point refuses the shape before any launch and the
    operator raises the library's error with the entry point's name."""
    rs = np.random.RandomState(3)
    col, ss, st = format_maps([make_maps(rs, "random", 1, 3, 30, S1)])
    loc = interior(rs, 2 * 4 * 3, [11], [4], 0.01, 0.99).reshape(1, 2, 4, 3, 2)
    w = rs.uniform(0, 1, (1, 2, 4, 3, 4, 3)).astype(F)
    from simpb_amd.plugin import ops
    f, l, wt = (dev(t).requires_grad_() for t in (col, loc, w))
    out = ops.deformable_aggregation_function(f, dev(ss), dev(st), l, wt)
    assert S.bound_b(out.detach().cpu().numpy(), S.daf(col, ss, st, loc, w)[0]) <= 1.0
    with pytest.raises(RuntimeError, match="simpb_deformable_aggregation_backward failed: SIMPB_EINVAL"):
        out.sum().backward()
    torch.cuda.synchronize()
    assert f.grad is None and l.grad is None and wt.grad is None


# ============================================================================================ 2D: msda_grouped_bwd
HEAD_CH = [(64, 4), (32, 8), (8, 32), (4, 64), (1, 256)]
LVL_PTS = [(S1, 4), (S1[:1], 1), (S1 + [(2, 2)], 8), (S2, 1)]
FAR = [1e30, -1e30, 3e38, -3e38, np.inf, -np.inf, np.nan, 3.0, -2.0]
QC = {(6, 23): [0, 0, 1, 1, 2, 2, -1, 4, 4, 5, 5, 7, -1, 0, 1, 2, 4, 5, -1, 0, 1, 2, 4],     # camera 3 has no query; 7 >= cams
      (1, 23): [0, 0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, -1, 0, 0, 0, 0, 0, -1, 0, 0, 0, 0],     # 1 >= cams
      (6, 1): [4], (1, 1): [0]}


def _d_cases():
    out = []
    for i, (heads, ch) in enumerate(HEAD_CH):
        for j in range(len(LVL_PTS)):
            k = i * len(LVL_PTS) + j
            out.append((heads, ch, j, (6, 1)[(i + j) % 2], (1, 2)[(i + j // 2) % 2], 1 if k % 5 == 4 else 23,
                        ("random", "ones", "random", "onehot")[k % 4]))
    return out


D_CASES = _d_cases()


def marks2d(n):
    """marks(n), and outside [0, 1]: the band beyond the map, and the pixels -1 and n themselves."""
    return marks(n) + [F(v) for v in (-0.25 / n, 1 + 0.25 / n, -0.5 / n, 1 + 0.5 / n)]


def value_maps(rs, content, bs, cams, heads, ch, shapes):
    maps = make_maps(rs, content, bs, cams, heads * ch, shapes)
    v = np.concatenate([m.reshape(bs, cams, heads * ch, -1).transpose(0, 1, 3, 2) for m in maps], 2)
    return np.ascontiguousarray(v).reshape(bs, cams, -1, heads, ch)


@functools.lru_cache(maxsize=None)
def d_case(heads, ch, j, cams, bs, nq, content):
    shapes, pts = LVL_PTS[j]
    rs = np.random.RandomState(zlib.crc32(f"bwd2d {heads} {ch} {j} {cams} {bs} {nq} {content}".encode()))
    value = value_maps(rs, content, bs, cams, heads, ch, shapes)
    L = len(shapes)
    loc = np.zeros((bs, nq, heads, L, pts, 2), F)
    slots = bs * nq * heads * pts
    for l, (h, w) in enumerate(shapes):
        marked = spread(cross([[(h, w)]], marks2d), slots // 2, seed=l)
        loc[:, :, :, l] = interleave(interior(rs, slots - slots // 2, [w], [h], -0.05, 1.05), marked).reshape(bs, nq, heads, pts, 2)
    if nq > len(FAR):
        for q, far in enumerate(FAR):          # one coordinate of every sample of head q of slot q
            loc[:, q, q % heads, :, :, q % 2] = far
    attn = rs.uniform(-1, 1, (bs, nq, heads, L, pts)).astype(F)
    attn.reshape(-1)[::5] = 0.0
    if heads > 1:
        attn[:, :, heads - 1] *= F(2.0 ** -10)
    qc = np.array(QC[cams, nq], np.int32)
    gout = low_block(rs, (bs, nq, heads * ch))
    return dict(value=value, shapes=shapes, loc=loc, attn=attn, qc=qc, gout=gout,
                want=G.msda_grad(value, shapes, loc, attn, qc, gout), dims=(bs, cams, value.shape[2], heads, ch, L, pts, nq))


def shape_tables(shapes):
    ss = torch.tensor(shapes, dtype=torch.long)
    return ss, torch.cat([ss.new_zeros(1), ss.prod(1).cumsum(0)[:-1]])


def contributes(c):
    """[bs, nq, heads, L, P]: the sample is finite, within a pixel of its map and belongs to a camera group."""
    loc = c["loc"].astype(np.float64)
    out = np.zeros(loc.shape[:-1], bool)
    for l, (h, w) in enumerate(c["shapes"]):
        with np.errstate(invalid="ignore", over="ignore"):
            px, py = loc[:, :, :, l, :, 0] * w - 0.5, loc[:, :, :, l, :, 1] * h - 0.5
            out[:, :, :, l] = np.isfinite(px) & np.isfinite(py) & (px > -2) & (px < w + 1) & (py > -2) & (py < h + 1)
    return out & (c["qc"] >= 0)[None, :, None, None, None]


def msda_autograd(c, gout, need=(True, True, True), transform=None):
    from simpb_amd.plugin import ops
    v, l, a = (dev(c[k]).requires_grad_(n) for k, n in zip(("value", "loc", "attn"), need))
    ss, lsi = shape_tables(c["shapes"])
    with guarded() as g:
        out = ops.ms_deform_attn_grouped(v, ss.cuda(), lsi.cuda(), l, a if transform is None else transform(a), dev(c["qc"]))
        g.holds(out)
    if gout is None:
        out.sum().backward()
    else:
        out.backward(gout)
    torch.cuda.synchronize()
    return v.grad, l.grad, a.grad


def msda_direct(c):
    from simpb_amd import _lib
    bs, cams, nv, heads, ch, L, pts, nq = c["dims"]
    gv, gl, ga = Padded(c["value"].shape), Padded(c["loc"].shape), Padded(c["attn"].shape)
    ss, lsi = shape_tables(c["shapes"])
    keep = [dev(c["value"]), ss.cuda(), lsi.cuda(), dev(c["loc"]), dev(c["attn"]), dev(c["qc"]), dev(c["gout"])]
    status = _lib.lib().simpb_ms_deform_attn_grouped_backward(gv.ptr(), gl.ptr(), ga.ptr(), *(ptr(t) for t in keep), bs, cams, nv, heads,
                                                              ch, L, pts, nq, stream())
    torch.cuda.synchronize()
    assert status == 0, status
    return gv.result("g_value"), gl.result("g_loc"), ga.result("g_attn")


def msda_asserts(name, c, gv, gl, ga):
    want = c["want"]
    gv, gl, ga = gv.cpu().numpy(), gl.cpu().numpy(), ga.cpu().numpy()
    for tag, got in (("g_value", gv), ("g_loc", gl), ("g_attn", ga)):
        check(f"{name} {tag}", got, want[tag])
    off = ~contributes(c)
    assert bits_zero(gl[off]).all() and bits_zero(ga[off]).all(), (name, "a capacity slot or a far / non-finite sample has a gradient")
    assert bits_zero(gv[want["g_value"]["count"] == 0]).all(), (name, "a token no sample touches has a gradient")
    cams = gv.shape[1]
    for cam in set(range(cams)) - set(np.minimum(c["qc"][c["qc"] >= 0], cams - 1).tolist()):
        assert bits_zero(gv[:, cam]).all(), (name, "a camera without a query has a gradient", cam)


@pytest.mark.gpu
@pytest.mark.parametrize("heads,ch,j,cams,bs,nq,content", D_CASES)
def test_2d_backward(heads, ch, j, cams, bs, nq, content):
    c = d_case(heads, ch, j, cams, bs, nq, content)
    name = f"2D h{heads}x{ch} L{len(c['shapes'])} P{LVL_PTS[j][1]} cams{cams} bs{bs} nq{nq} {content}"
    auto = msda_autograd(c, dev(c["gout"]))
    msda_asserts(name + " autograd", c, *auto)
    direct = msda_direct(c)
    msda_asserts(name + " direct", c, *direct)
    assert same_bits(auto[1], direct[1]) and same_bits(auto[2], direct[2]), (name, "g_loc / g_attn differ between two launches")


@functools.lru_cache(maxsize=None)
def d_single(content):
    rs = np.random.RandomState(17 + len(content))
    shapes, heads, ch = [(4, 11)], 8, 32
    value = value_maps(rs, content, 1, 1, heads, ch, shapes)
    loc = np.tile(np.array(ONE_LOC, F), (1, 1, heads, 1, 1, 1))
    attn = np.tile(np.array([1.5, 0.75, 0.375, 3.0, -1.5, -0.75, 0.0, 1.0], F).reshape(1, 1, heads, 1, 1), (1, 1, 1, 1, 1))
    qc = np.zeros(1, np.int32)
    gout = low_block(rs, (1, 1, heads * ch))
    return dict(value=value, shapes=shapes, loc=loc, attn=attn, qc=qc, gout=gout, want=G.msda_grad(value, shapes, loc, attn, qc, gout),
                dims=(1, 1, value.shape[2], heads, ch, 1, 1, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["random", "onehot"])
def test_2d_backward_single_contribution(content):
    """nq = P = L = 1: one addend per touched element of g_value. attention weight * tap weight is exact (few bits each), so
    the addend is one rounding from float64: within 2 ulp."""
    c = d_single(content)
    gv, gl, ga = msda_direct(c)
    msda_asserts(f"2D single {content}", c, gv, gl, ga)
    assert (c["want"]["g_value"]["count"] <= 1).all() and (c["want"]["g_value"]["count"] == 1).sum() == 4 * 256
    u = ulps(gv.cpu().numpy(), c["want"]["g_value"]["want"])
    print(f"FIG 2D single {content} g_value ulp={u:.2f}")
    assert u <= 2.0, u


def d_wrapper_case():
    return d_case(8, 32, 0, 6, 1, 23, "random")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sum", "fp16", "loc_only", "strided_weights"])
def test_2d_wrapper(kind):
    """As test_3d_wrapper, for ms_deform_attn_grouped."""
    c = d_wrapper_case()
    name = f"2D wrapper {kind}"
    args = [c[k] for k in ("value", "shapes", "loc", "attn", "qc")]
    if kind == "sum":
        want = G.msda_grad(*args, np.ones_like(c["gout"]))
        got = msda_autograd(c, None)
    elif kind == "fp16":
        g16 = c["gout"].astype(np.float16)
        want = G.msda_grad(*args, g16.astype(F))
        got = msda_autograd(c, dev(g16))
    elif kind == "loc_only":
        want = c["want"]
        got = msda_autograd(c, dev(c["gout"]), need=(False, True, False))
        assert got[0] is None and got[2] is None
    else:
        want = c["want"]
        wide = np.zeros(c["attn"].shape[:-1] + (2 * c["attn"].shape[-1],), F)
        wide[..., ::2] = c["attn"]
        got = msda_autograd(dict(c, attn=wide), dev(c["gout"]), transform=lambda t: t[..., ::2])
        assert bits_zero(got[2][..., 1::2].cpu().numpy()).all()
        got = (got[0], got[1], got[2][..., ::2])
    for tag, g in zip(("g_value", "g_loc", "g_attn"), got):
        if g is not None:
            check(f"{name} {tag}", g.cpu().numpy(), want[tag])


@pytest.mark.gpu
def test_2d_backward_refuses_what_only_the_forward_takes():
    """heads * ch = 128: the forward's generic instance serves it, the backward's entry point refuses it before any launch
    and the operator raises the library's error with the entry point's name."""
    rs = np.random.RandomState(5)
    c = dict(value=value_maps(rs, "random", 1, 1, 4, 32, S1), shapes=S1, qc=np.zeros(3, np.int32),
             loc=interior(rs, 3 * 4 * 4 * 2, [11, 6, 3, 1], [4, 2, 1], 0.01, 0.99).reshape(1, 3, 4, 4, 2, 2),
             attn=rs.uniform(0, 1, (1, 3, 4, 4, 2)).astype(F))
    from simpb_amd.plugin import ops
    v, l, a = (dev(c[k]).requires_grad_() for k in ("value", "loc", "attn"))
    ss, lsi = shape_tables(S1)
    out = ops.ms_deform_attn_grouped(v, ss.cuda(), lsi.cuda(), l, a, dev(c["qc"]))
    assert S.bound_b(out.detach().cpu().numpy(), S.msda(c["value"][:, 0], S1, c["loc"], c["attn"])[0]) <= 1.0
    with pytest.raises(RuntimeError, match="simpb_ms_deform_attn_grouped_backward failed: SIMPB_EINVAL"):
        out.sum().backward()
    torch.cuda.synchronize()
    assert v.grad is None and l.grad is None and a.grad is None


@pytest.mark.gpu
def test_2d_backward_without_queries():
    """nq = 0: the forward launches nothing and the backward returns a zero g_value and two empty gradients."""
    from simpb_amd.plugin import ops
    rs = np.random.RandomState(6)
    v = dev(value_maps(rs, "random", 2, 6, 8, 32, S1)).requires_grad_()
    l = torch.zeros(2, 0, 8, 4, 4, 2, device="cuda", requires_grad=True)
    a = torch.zeros(2, 0, 8, 4, 4, device="cuda", requires_grad=True)
    ss, lsi = shape_tables(S1)
    out = ops.ms_deform_attn_grouped(v, ss.cuda(), lsi.cuda(), l, a, torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert tuple(out.shape) == (2, 0, 256)
    out.sum().backward()
    torch.cuda.synchronize()
    assert tuple(v.grad.shape) == tuple(v.shape) and bits_zero(v.grad.cpu().numpy()).all()
    assert tuple(l.grad.shape) == tuple(l.shape) and tuple(a.grad.shape) == tuple(a.shape)


@pytest.mark.gpu
def test_entry_points_take_their_accepted_corners():
    """The corners the validation lets through (tests/test_sampler_grad_ref_host.py holds the refusals on the CPU): C = 64 with
    G = 1, C = 192 with G = 2 and P * K = 128 in 3D; ch = 4 and ch = 256 in 2D. Their results are held by the cases above;
    here only the status."""
    for shape in ("c64_g1", "c192_g2", "pk128"):
        daf_direct(t_case(shape, 1, 1, "random"))
    for heads, ch in ((64, 4), (1, 256)):
        msda_direct(d_case(*next(d for d in D_CASES if d[:2] == (heads, ch))))
