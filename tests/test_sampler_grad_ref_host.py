"""CPU: the float64 statement of the two sampler gradients (tests/sampler_grad_ref.py) tied to what is pinned already --
float64 autograd through the oracle's forwards, central differences of tests/sampler_ref.py, and the edge rules stated as
facts -- then the fp32 oracle's autograd on every GPU case of tests/test_samplers_backward_float64.py (it measures
KAPPA_BWD), the condition on those cases that keeps `jump` from becoming a place to hide, and the argument validation of the
two backward entry points, which runs before any HIP call."""
import ctypes

import numpy as np
import torch

from tests import sampler_grad_ref as G
from tests import sampler_ref as S
from tests import test_samplers_backward_float64 as B
from tests.test_samplers_float64 import S1, S2, format_maps, make_maps

F = np.float32


def _R():
    from oracle import simpb_ref
    return simpb_ref


def t(x, dtype=None):
    out = torch.from_numpy(np.ascontiguousarray(x))
    return out if dtype is None else out.to(dtype)


# ------------------------------------------------------------------------------------------------ the oracle's autograd
def oracle_daf_grad(c, dtype):
    """(g_feat, g_loc, g_w) by torch autograd through oracle.deformable_aggregation. Non-finite locations are handed over as
    -1: the gate drops both, and the oracle's masked arithmetic would multiply NaN by zero."""
    loc = np.where(np.isfinite(c["loc"]).all(-1, keepdims=True), c["loc"], F(-1))
    f, l, w = (t(x, dtype).requires_grad_() for x in (c["col"], loc, c["w"]))
    out = _R().deformable_aggregation(f, t(c["ss"]), t(c["st"]), l, w)
    if not out.requires_grad:      # every sample gated out: the oracle returns its zeros untouched
        return tuple(np.zeros(x.shape) for x in (f, l, w))
    out.backward(t(c["gout"], dtype))
    return f.grad.numpy(), l.grad.numpy(), w.grad.numpy()


def oracle_msda_grad(c, dtype):
    """(g_value, g_loc, g_attn) by torch autograd through oracle.ms_deform_attn, camera group by camera group. Far and
    non-finite locations are handed over as 3.0 (outside every map; grid_sample gives NaN for the non-finite ones)."""
    with np.errstate(invalid="ignore"):
        tame = np.isfinite(c["loc"]) & (np.abs(c["loc"]) < 1e3)
    v, l, a = t(c["value"], dtype).requires_grad_(), t(np.where(tame, c["loc"], F(3)), dtype).requires_grad_(), t(c["attn"], dtype).requires_grad_()
    cams, qc = c["value"].shape[1], c["qc"]
    total = None
    for cam in range(cams):
        q = np.nonzero((qc >= 0) & (np.minimum(qc, cams - 1) == cam))[0]
        if q.size:
            out = _R().ms_deform_attn(v[:, cam], torch.tensor(c["shapes"]), l[:, q], a[:, q])
            part = (out * t(c["gout"][:, q], dtype)).sum()
            total = part if total is None else total + part
    if total is None:
        return tuple(np.zeros(c[k].shape) for k in ("value", "loc", "attn"))
    total.backward()
    return v.grad.numpy(), l.grad.numpy(), a.grad.numpy()


# ------------------------------------------------------------------------------------- random cases away from integers
def random_daf(seed=0):
    rs = np.random.RandomState(seed)
    bs, A, P, K, C, Gr = 2, 3, 2, 4, 6, 3
    col, ss, st = format_maps([make_maps(rs, "random", bs, 2, C, S1), make_maps(rs, "random", bs, 2, C, S2)])
    # the oracle rounds its pixel to fp32 whatever the dtype of its operands (`.float()`, as the reference's kernel does):
    # its fractions and tap weights are fp32 too. On multiples of 2^-6 the pixel, the fractions and their products are fp32
    # numbers, and the oracle in float64 is a float64 statement
    loc = B.interior(rs, bs * A * P * K, [w for _, w in S1 + S2], [h for h, _ in S1 + S2], -0.2, 1.2, grid=2 ** 6).reshape(bs, A, P, K, 2)
    w = rs.standard_normal((bs, A, P, K, 4, Gr)).astype(F)
    return dict(col=col, ss=ss, st=st, loc=loc, w=w, gout=rs.standard_normal((bs, A, C)).astype(F))


def random_msda(seed=1):
    rs = np.random.RandomState(seed)
    bs, cams, heads, ch, nq, P = 2, 3, 2, 4, 7, 2
    value = B.value_maps(rs, "random", bs, cams, heads, ch, S1)
    loc = np.zeros((bs, nq, heads, 4, P, 2), F)
    for l, (h, w) in enumerate(S1):
        loc[:, :, :, l] = B.interior(rs, bs * nq * heads * P, [w], [h], -0.3, 1.3).reshape(bs, nq, heads, P, 2)
    attn = rs.standard_normal((bs, nq, heads, 4, P)).astype(F)
    return dict(value=value, shapes=S1, loc=loc, attn=attn, qc=np.array([0, 1, -1, 2, 5, 0, 1], np.int32),
                gout=rs.standard_normal((bs, nq, heads * ch)).astype(F))


def oracle_daf_grad_by_grid_sample(c):
    """The 3D operator written with the oracle's ms_deform_attn, float64 throughout: a camera's tokens are the value, the
    groups the heads, the anchors the queries; every head samples the same locations, and a gated sample has its weights
    multiplied by zero. (oracle.deformable_aggregation keeps pixel, fractions and tap weights in fp32 whatever its operands
    are, as the reference's kernel does, so the gradient that flows back through them is rounded to fp32.)"""
    f, l, w = (t(c[k], torch.float64).requires_grad_() for k in ("col", "loc", "w"))
    bs, _, C = f.shape
    A, P, K = l.shape[1:4]
    L, Gr = w.shape[-2:]
    keep = t(B.gate(c["loc"]).astype(np.float64))
    out = 0
    for cam in range(K):
        shapes = [tuple(int(v) for v in hw) for hw in c["ss"][cam]]
        start, nv = int(c["st"][cam, 0]), sum(h * wd for h, wd in shapes)
        value = f[:, start:start + nv].reshape(bs, nv, Gr, C // Gr)
        loc = l[:, :, None, None, :, cam].expand(bs, A, Gr, L, P, 2)
        attn = (w[:, :, :, cam] * keep[:, :, :, cam, None, None]).permute(0, 1, 4, 3, 2)
        out = out + _R().ms_deform_attn(value, torch.tensor(shapes), loc, attn)
    out.backward(t(c["gout"], torch.float64))
    return f.grad.numpy(), l.grad.numpy(), w.grad.numpy()


def agrees(got, ref, rel=1e-12):
    return bool((np.abs(got - ref["want"]) <= rel * ref["abs_sum"] + 1e-300).all())


def test_statement_agrees_with_float64_autograd_of_the_oracle():
    c = random_daf()
    want = G.daf_grad(c["col"], c["ss"], c["st"], c["loc"], c["w"], c["gout"])
    assert B.gate(c["loc"]).sum() > 20 and (~B.gate(c["loc"])).sum() > 10
    for tag, got in zip(("g_feat", "g_loc", "g_w"), oracle_daf_grad_by_grid_sample(c)):
        assert agrees(got, want[tag]), tag
    # through oracle.deformable_aggregation: the multiples of 2^-6 make its fp32 pixel, fractions and tap weights exact, so
    # g_feat and g_w are float64 statements; g_loc flows back through those fp32 tensors and is rounded there
    got = oracle_daf_grad(c, torch.float64)
    assert agrees(got[0], want["g_feat"]) and agrees(got[2], want["g_w"])
    assert agrees(got[1], want["g_loc"], rel=2.0 ** -22)
    assert (want["g_loc"]["jump"] == 0).all()
    c = random_msda()
    want = G.msda_grad(c["value"], c["shapes"], c["loc"], c["attn"], c["qc"], c["gout"])
    for tag, got in zip(("g_value", "g_loc", "g_attn"), oracle_msda_grad(c, torch.float64)):
        assert agrees(got, want[tag]), tag
    assert (want["g_loc"]["jump"] == 0).all()
    assert (want["g_loc"]["want"][:, 2] == 0).all() and (want["g_attn"]["want"][:, 2] == 0).all()     # query_cam < 0
    assert (want["g_loc"]["want"][:, 4] != 0).any()                                                   # query_cam >= cams: the last camera


def test_statement_agrees_with_central_differences_of_the_forward_statement():
    """g_loc and g_w / g_attn of a handful of interior samples: d/d(input) of sum(g_out * forward) by central differences of
    sampler_ref.daf / sampler_ref.msda. The forwards are linear in the weights and, inside a cell, in the location."""
    h = 2.0 ** -13
    c = random_daf(2)
    c["loc"] = (np.round(c["loc"].astype(np.float64) * 2 ** 14) / 2 ** 14).astype(F)       # loc +- h is an fp32 number
    want = G.daf_grad(c["col"], c["ss"], c["st"], c["loc"], c["w"], c["gout"])
    fwd = lambda loc, w: float((S.daf(c["col"], c["ss"], c["st"], loc, w)[0] * c["gout"]).sum())   # noqa: E731
    # samples whose pixel stays at least 0.01 from every integer on every level of both pyramids
    sizes = np.array([s for p in (S1, S2) for hw in p for s in hw], np.float64)
    frac = np.abs((c["loc"].astype(np.float64)[..., None] * sizes - 0.5) - np.rint(c["loc"].astype(np.float64)[..., None] * sizes - 0.5))
    idx = [i for i in zip(*np.nonzero(B.gate(c["loc"]) & (frac.min((-1, -2)) >= 0.01)))][:5]
    assert len(idx) == 5
    for i in idx:
        for axis in (0, 1):
            up, dn = c["loc"].copy(), c["loc"].copy()
            up[i + (axis,)] += F(h)
            dn[i + (axis,)] -= F(h)
            cd = (fwd(up, c["w"]) - fwd(dn, c["w"])) / (2 * h)
            assert abs(cd - want["g_loc"]["want"][i + (axis,)]) <= 1e-9 * max(1.0, want["g_loc"]["abs_sum"][i + (axis,)]), (i, axis)
        j = i + (1, 2)
        up, dn = c["w"].astype(np.float64), c["w"].astype(np.float64)
        up[j] += 0.5
        dn[j] -= 0.5
        assert abs(fwd(c["loc"], up) - fwd(c["loc"], dn) - want["g_w"]["want"][j]) <= 1e-9 * max(1.0, want["g_w"]["abs_sum"][j]), j
    c = random_msda(3)
    c["loc"] = (np.round(c["loc"].astype(np.float64) * 2 ** 14) / 2 ** 14).astype(F)
    c["qc"][:] = 1
    want = G.msda_grad(c["value"], c["shapes"], c["loc"], c["attn"], c["qc"], c["gout"])
    fwd = lambda loc, a: float((S.msda(c["value"][:, 1], c["shapes"], loc, a)[0] * c["gout"]).sum())   # noqa: E731
    done = 0
    for i in zip(*np.nonzero(B.contributes(c))):
        size = np.array(c["shapes"][i[3]][::-1], np.float64)
        px = c["loc"][i].astype(np.float64) * size - 0.5
        if (np.abs(px - np.rint(px)) < 0.05).any() or (px < 0).any() or (px > size - 1).any():
            continue
        for axis in (0, 1):
            up, dn = c["loc"].copy(), c["loc"].copy()
            up[i + (axis,)] += F(h)
            dn[i + (axis,)] -= F(h)
            cd = (fwd(up, c["attn"]) - fwd(dn, c["attn"])) / (2 * h)
            assert abs(cd - want["g_loc"]["want"][i + (axis,)]) <= 1e-9 * max(1.0, want["g_loc"]["abs_sum"][i + (axis,)]), (i, axis)
        up, dn = c["attn"].astype(np.float64), c["attn"].astype(np.float64)
        up[i] += 0.5
        dn[i] -= 0.5
        assert abs(fwd(c["loc"], up) - fwd(c["loc"], dn) - want["g_attn"]["want"][i]) <= 1e-9 * max(1.0, want["g_attn"]["abs_sum"][i]), i
        done += 1
        if done == 5:
            break
    assert done == 5


# ------------------------------------------------------------------------------------------------- edge rules as facts
def test_gated_far_and_non_finite_samples_give_exact_zeros():
    c = B.t_case("c64_g2", 1, 7, "gated")
    for tag in ("g_feat", "g_loc", "g_w"):
        for k, v in c["want"][tag].items():
            assert (v == 0).all(), (tag, k)
    c = B.t_case("shipped", 2, 7, "random")
    off = ~B.gate(c["loc"])
    assert off.sum() > 50 and (~np.isfinite(c["loc"])).any()
    for tag in ("g_loc", "g_w"):
        for k, v in c["want"][tag].items():
            assert (v[off] == 0).all(), (tag, k)
    c = B.d_wrapper_case()
    off = ~B.contributes(c)
    assert off[:, :len(B.FAR)].sum() >= len(B.FAR) and off[:, c["qc"] < 0].all()
    for tag in ("g_loc", "g_attn"):
        for k, v in c["want"][tag].items():
            assert (v[off] == 0).all(), (tag, k)
    assert (c["want"]["g_value"]["want"][:, 3] == 0).all() and (c["want"]["g_value"]["count"][:, 3] == 0).all()    # camera 3: no query


def test_constant_maps_move_only_in_the_border_band():
    """On a map of ones the sample is the sum of its valid tap weights: 1 wherever the four taps are inside, so g_loc is zero
    there, and falling towards the border inside the half-pixel band, so g_loc is not."""
    rs = np.random.RandomState(4)
    H, W, C = 4, 11, 4
    col, ss, st = format_maps([make_maps(rs, "ones", 1, 1, C, [(H, W)])])
    xs = np.array([1.5 / W, 0.3, 0.5, 0.77, 1 - 1.5 / W, 0.2 / W, 1 - 0.2 / W, 0.4], F)      # 5 inside, 2 in the band, 1 inside
    ys = np.array([1.5 / H, 0.3, 0.5, 0.77, 1 - 1.5 / H, 0.4, 0.6, 0.1 / H], F)              # ...                   1 in the band
    loc = np.stack([xs, ys], -1).reshape(1, 1, 8, 1, 2)
    w, gout = np.ones((1, 1, 8, 1, 1, 1), F), np.ones((1, 1, C), F)
    r = G.daf_grad(col, ss, st, loc, w, gout)["g_loc"]
    g = r["want"][0, 0, :, 0]
    assert (np.abs(g[:5]) + r["jump"][0, 0, :5, 0] <= 1e-12).all()       # (at an interior centre both one-sided values are zero)
    assert g[5, 0] > 1 and g[6, 0] < -1 and g[7, 1] > 1
    assert abs(g[5, 1]) <= 1e-12 and abs(g[7, 0]) <= 1e-12
    value = col.reshape(1, 1, H * W, 1, C)
    r = G.msda_grad(value, [(H, W)], loc.reshape(1, 8, 1, 1, 1, 2), np.ones((1, 8, 1, 1, 1), F), np.zeros(8, np.int32), np.ones((1, 8, C), F))
    g = r["g_loc"]["want"].reshape(8, 2)
    assert (np.abs(g[:5]) <= 1e-12).all() and g[5, 0] > 1 and g[6, 0] < -1 and g[7, 1] > 1


def test_one_hot_maps_name_the_samples_that_touch_the_hot_pixel():
    """A one-hot map: g_w / g_attn is non-zero exactly for the samples one of whose taps is the hot pixel (with a non-zero
    weight), and g_feat / g_value -- which does not read the map -- lands on the four taps of each sample."""
    rs = np.random.RandomState(8)
    H, W, C = 4, 11, 4
    col = np.zeros((1, H * W, C), F)
    col[0, 1 * W + 6] = 1.0                                                        # hot pixel (y 1, x 6)
    ss, st = np.array([[[H, W]]], np.int32), np.array([[0]], np.int32)
    px = np.array([(5.5, 0.5), (6.0, 1.0), (6.75, 1.25), (7.5, 1.0), (3.0, 1.0), (6.0, 2.5), (5.0, 1.0), (6.5, 0.25)])
    loc = ((px + 0.5) / np.array([W, H])).astype(F).reshape(1, 1, 8, 1, 2)
    r = G.daf_grad(col, ss, st, loc, np.ones((1, 1, 8, 1, 1, 1), F), np.ones((1, 1, C), F))
    touched = np.array([True, True, True, False, False, False, False, True])      # (7.5: taps 7, 8; (6, 2.5): rows 2, 3; (5, 1): x weight 0)
    assert np.array_equal(r["g_w"]["want"].reshape(8) != 0, touched)
    gf = r["g_feat"]["want"][0, :, 0].reshape(H, W)
    assert gf[1, 6] > 0 and gf[3, 0] == 0 and abs(gf.sum() - 8.0) <= 1e-9          # every sample's four tap weights sum to 1
    assert (r["g_feat"]["count"][r["g_feat"]["want"] != 0] > 0).all() and r["g_feat"]["count"][0, 3 * W, 0] == 0


def test_at_an_exact_centre_the_one_sided_derivatives_bracket_want():
    rs = np.random.RandomState(9)
    H, W, C = 4, 11, 3
    col, ss, st = format_maps([make_maps(rs, "random", 1, 1, C, [(H, W)])])
    loc = np.array([(5 + 0.5) / W, 0.40625], F).reshape(1, 1, 1, 1, 2)            # x: the centre of column 5 (to fp32 rounding)
    w, gout = np.ones((1, 1, 1, 1, 1, 1), F), rs.standard_normal((1, 1, C)).astype(F)
    r = G.daf_grad(col, ss, st, loc, w, gout)["g_loc"]
    assert r["jump"][0, 0, 0, 0, 0] > 0 and r["jump"][0, 0, 0, 0, 1] == 0
    h = 2.0 ** -10
    fwd = lambda x: float((S.daf(col, ss, st, np.array([x, loc[0, 0, 0, 0, 1]], F).reshape(loc.shape), w)[0] * gout).sum())   # noqa: E731
    x0 = float(loc[0, 0, 0, 0, 0])
    left = (fwd(x0 - h) - fwd(x0 - 2 * h)) / h               # slopes inside the two cells, away from the centre
    right = (fwd(x0 + 2 * h) - fwd(x0 + h)) / h
    want, jump = r["want"][0, 0, 0, 0, 0], r["jump"][0, 0, 0, 0, 0]
    assert abs(min(left, right) - (want - jump)) <= 1e-6 and abs(max(left, right) - (want + jump)) <= 1e-6
    assert abs(left - right) > 1e-3


# ------------------------------------------------------------------------------- every GPU case: jump, and the fp32 oracle
def all_cases():
    """(name, case, gradient names, oracle): every GPU case of tests/test_samplers_backward_float64.py."""
    for case in B.T_CASES:
        yield "3D " + " ".join(map(str, case)), B.t_case(*case), ("g_feat", "g_loc", "g_w"), oracle_daf_grad
    for content in ("random", "onehot"):
        yield f"3D single {content}", B.t_single(content), ("g_feat", "g_loc", "g_w"), oracle_daf_grad
    for case in B.D_CASES:
        yield "2D " + " ".join(map(str, case)), B.d_case(*case), ("g_value", "g_loc", "g_attn"), oracle_msda_grad
    for content in ("random", "onehot"):
        yield f"2D single {content}", B.d_single(content), ("g_value", "g_loc", "g_attn"), oracle_msda_grad


def oracle_reference(c):
    """The statement the fp32 oracle is measured against. 3D: the case's own (the oracle takes the kernels' route to the
    pixel). 2D: the same gradients with the eps of grid_sample's route to the pixel (sampler_grad_ref.grid_sample_pixel) in
    shift_sum and in what counts as ambiguous."""
    if "value" not in c:
        return c["want"]
    return G.msda_grad(c["value"], c["shapes"], c["loc"], c["attn"], c["qc"], c["gout"], pixel=G.grid_sample_pixel)


def test_at_least_half_of_every_case_has_no_jump():
    for name, c, _, _ in all_cases():
        jump = c["want"]["g_loc"]["jump"]
        assert (jump == 0).sum() * 2 >= jump.size, (name, int((jump == 0).sum()), jump.size)
    # and the hand-placed half does reach the discontinuities
    assert (B.t_case("shipped", 2, 7, "random")["want"]["g_loc"]["jump"] > 0).sum() > 50
    assert (B.d_wrapper_case()["want"]["g_loc"]["jump"] > 0).sum() > 50


def test_fp32_oracle_stays_under_half_of_the_bounds():
    """The oracle's autograd in float32 on the CPU over every GPU case: its figure against (b) and the kappa it needs for
    (e), per gradient. KAPPA_BWD is twice the largest; the oracle stays under half of each bound."""
    worst_b, worst_k = 0.0, 0.0
    for name, c, tags, oracle in all_cases():
        ref = oracle_reference(c)
        for tag, got in zip(tags, oracle(c, torch.float32)):
            assert np.isfinite(got).all(), (name, tag)
            b, k = G.bound_b(got, ref[tag]), G.kappa_needed(got, ref[tag])
            print(f"FIG oracle {name} {tag} b={b:.3f} e={G.bound_e(got, ref[tag], B.KAPPA_BWD):.3f} kappa={k:.2f}")
            worst_b, worst_k = max(worst_b, b), max(worst_k, k)
    print(f"FIG oracle worst b={worst_b:.3f} kappa={worst_k:.2f} KAPPA_BWD={B.KAPPA_BWD}")
    assert worst_b <= 0.5
    assert 2 * worst_k <= B.KAPPA_BWD, (worst_k, B.KAPPA_BWD)


# ------------------------------------------------------------------------------------------------- argument validation
def test_backward_entry_points_validate_before_any_hip_call():
    """As tests/test_stream_activity_host.py: no device in the process, so only the refusals are asserted here -- past its
    validation an entry point makes HIP calls. The accepted corners (C = 64 with G = 1, C = 192 with G = 2, P * K = 128;
    ch = 4, ch = 256) are launched by tests/test_samplers_backward_float64.py::test_entry_points_take_their_accepted_corners."""
    from simpb_amd import _lib, build
    build.build_extension()
    h = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)
    P = lambda n, v: [v] * n   # noqa: E731
    # simpb_deformable_aggregation_backward: 9 pointers, bs, cams, num_feat, C, L, A, P, G, stream
    daf = h.simpb_deformable_aggregation_backward
    assert daf(*P(9, null), 1, 6, 360, 256, 4, 7, 13, 8, null) == 1
    for i in range(9):
        assert daf(*(P(i, one) + [null] + P(8 - i, one)), 1, 6, 360, 256, 4, 7, 13, 8, null) == 1, i
    assert daf(*P(9, one), 1, 6, 360, 96, 4, 7, 13, 3, null) == 1          # C % 64
    assert daf(*P(9, one), 1, 6, 360, 320, 4, 7, 13, 10, null) == 1        # C > 256
    assert daf(*P(9, one), 1, 6, 360, 256, 4, 7, 13, 16, null) == 1        # gd = 16
    assert daf(*P(9, one), 1, 3, 360, 256, 4, 7, 43, 8, null) == 1         # P * K = 129
    assert daf(*P(9, one), 65536, 6, 360, 256, 4, 7, 13, 8, null) == 1     # batch_size beyond the grid's y
    assert daf(*P(9, one), 1, 6, 360, 256, 4, 7, 13, 7, null) == 1         # C % G
    assert daf(*P(9, one), 1, 6, 360, 256, 0, 7, 13, 8, null) == 1
    # simpb_ms_deform_attn_grouped_backward: 10 pointers, bs, cams, num_value, heads, ch, L, P, nq, stream
    msda = h.simpb_ms_deform_attn_grouped_backward
    assert msda(*P(10, null), 1, 6, 60, 8, 32, 4, 4, 23, null) == 1
    for i in range(10):
        assert msda(*(P(i, one) + [null] + P(9 - i, one)), 1, 6, 60, 8, 32, 4, 4, 23, null) == 1, i
    assert msda(*P(10, one), 1, 6, 60, 4, 32, 4, 4, 23, null) == 1         # heads * ch = 128
    assert msda(*P(10, one), 1, 6, 60, 8, 6, 4, 4, 23, null) == 1          # ch = 6
    assert msda(*P(10, one), 1, 6, 60, 8, 12, 4, 4, 23, null) == 1         # ch = 12
    assert msda(*P(10, one), 1, 6, 60, 8, 32, 4, 4, 0, null) == 1          # no query: the operator does not come here
    assert msda(*P(10, one), 65536, 6, 60, 8, 32, 4, 4, 23, null) == 1
