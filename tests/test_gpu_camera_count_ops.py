"""The one-launch 3D aggregation (csrc/deform_agg_fused.hip, simpb_dfa_fused_forward_rig) at 1..8 cameras, alone.

The cases are section B of tests/test_samplers_float64.py with n cameras (tests/camera_count_cases.py): bs 3, 48 anchors, the
first ceil(n / 2) cameras on pyramid S1 and the others on S2, the "affine" and "scene" operand families, "random" and
"dominant" logits, f16 and f32 tokens, and three masks: none, all ones, one camera left per stream. Checked in that module's
two stages: the returned locations and weights against the float64 statement (weights <= 1e-6, locations within their own
fp32 bound, the gate equal on every anchor without an undecided sample, at most 2 % of the anchors left out -- the CPU test
tests/test_camera_count_host.py shows the reference alone stays inside that), then the aggregation on the kernel's own
operands under bounds (b) = 2e-5 * max(1, max |want|) and (e) with that module's KAPPA. Everything of a masked camera holds
NaN; outputs lie in sentinel-guarded buffers. Each test prints its figures (`FIG ...`) before it asserts."""
import numpy as np
import pytest
import torch

from tests import camera_count_cases as K
from tests import sampler_ref as S
from tests import test_samplers_float64 as T

pytestmark = pytest.mark.gpu


def operands(c, mask, tok):
    tokens, proj, cl = c["col"].copy(), c["proj"].copy(), c["cl"].copy()
    if mask is not None:      # nothing of a masked camera is read: its tokens, matrix and logits hold NaN
        for b, cam in zip(*np.nonzero(mask == 0)):
            lo, hi = c["st"][cam, 0], c["st"][cam, -1] + c["ss"][cam, -1].prod()
            tokens[b, lo:hi], proj[b, cam], cl[b, cam] = np.nan, np.nan, np.nan
    feat = T.dev(tokens, torch.float16 if tok == "f16" else torch.float32).contiguous()
    return feat, T.dev(proj), T.dev(cl)


def fused(c, mask, tok):
    from simpb_amd.plugin import ops
    feat, proj, cl = operands(c, mask, tok)
    with T.guarded() as g:
        out, loc, w = ops.dfa_fused(feat, T.dev(c["ss"]), T.dev(c["st"]), T.dev(c["anchor"]), T.dev(c["learn"]), T.dev(c["fix"]), proj,
                                    T.dev(c["wh"]), T.dev(c["fl"]), cl, K.GRP, want_operands=True,
                                    cam_valid=T.dev(mask) if mask is not None else None)
        g.holds(out, loc, w)
    return out, loc, w


@pytest.mark.parametrize("tok", ["f32", "f16"])
@pytest.mark.parametrize("mask_kind", K.MASKS)
@pytest.mark.parametrize("family,logits", K.OPS_CASES)
@pytest.mark.parametrize("n", K.OPS_CAMS)
def test_fused_aggregation_at_n_cameras(n, family, logits, mask_kind, tok):
    c = K.ops_case(n, family, logits)
    name = f"N{n} {family} {logits} {tok} {mask_kind}"
    mask = K.mask_of(mask_kind, n)
    out, loc, w = (t.cpu().numpy() for t in fused(c, mask, tok))
    assert np.isfinite(out).all() and np.isfinite(loc).all() and np.isfinite(w).all(), name
    # ---- stage 1: the operands against float64
    pts = K.masked_points(c, mask)
    want_w = S.dfa_weights(c["fl"], c["cl"], K.LVL, K.NPTS, K.GRP, mask)
    werr = float(np.abs(w - want_w).max())
    print(f"FIG {name} stage1 weights={werr:.2e}")
    assert werr <= 1e-6, (name, werr)
    off = np.zeros((c["bs"], n), bool) if mask is None else mask == 0
    sel = np.broadcast_to(off[:, None, None, :], loc.shape[:4])
    assert (loc[sel] == -1.0).all() and (w[sel] == 0.0).all(), name
    ref = pts["loc"]
    near = (pts["depth"] > 1e-3) & ~off[:, None, None, :]
    ratio = float((np.abs(loc - ref)[near] / pts["bound"][near]).max())
    und, left = K.anchors_left_out(pts, mask)
    keep = ~und.any(axis=(2, 3))
    print(f"FIG {name} stage1 loc={ratio:.3f} undecided={int(und.sum())} anchors_left_out={left}")
    assert ratio <= 1.0, (name, ratio)
    assert left <= 0.02 * c["bs"] * c["A"]
    assert np.array_equal(T.gate(loc)[keep], T.gate(ref)[keep]), name
    # ---- stage 2: the aggregation on the kernel's own operands (the gate is decided on identical numbers)
    T.check(name, out, *K.reference(c, c["col"], loc, w, mask))


def three_launches(c, mask, n):
    """simpb_dfa_points_cams + simpb_dfa_weights_cams + the drop-in operator on the same operands (fp32 tokens)."""
    from simpb_amd import _lib as L
    from simpb_amd.plugin import ops
    from simpb_amd.plugin.ops import _ptr as P, _stream
    lib = L.lib()
    feat, proj, cl = operands(c, mask, "f32")
    anchor, learn, fix, wh, fl = (T.dev(c[k]) for k in ("anchor", "learn", "fix", "wh", "fl"))
    cv = T.dev(mask) if mask is not None else None
    bs, a = c["bs"], c["A"]
    loc = torch.full((bs, a, K.NPTS, n, 2), float("nan"), device="cuda")
    w = torch.full((bs, a, K.NPTS, n, K.LVL, K.GRP), float("nan"), device="cuda")
    L.check(lib.simpb_dfa_points_cams(P(loc), None, P(anchor), P(learn), P(fix), P(proj), P(wh), bs, a, K.NFIX, K.NLEARN, n,
                                      P(cv) if cv is not None else None, _stream()), "simpb_dfa_points_cams")
    L.check(lib.simpb_dfa_weights_cams(P(w), P(fl), P(cl), bs, a, n, K.LVL, K.NPTS, K.GRP, P(cv) if cv is not None else None,
                                       _stream()), "simpb_dfa_weights_cams")
    out = ops.deformable_aggregation_function(feat, T.dev(c["ss"]), T.dev(c["st"]), loc, w)
    torch.cuda.synchronize()
    return out.reshape(bs, a, -1), loc, w


@pytest.mark.parametrize("mask_kind", ["none", "one_left"])
@pytest.mark.parametrize("n", K.OPS_CAMS)
def test_one_launch_equals_the_three_launch_route(n, mask_kind):
    c = K.ops_case(n, "scene", "random")
    mask = K.mask_of(mask_kind, n)
    want, want_loc, want_w = three_launches(c, mask, n)
    for tok in ("f32", "f16"):
        out, loc, w = fused(c, mask, tok)
        tol = 2e-5 * max(1.0, float(want.abs().max()))
        err, lerr, werr = float((out - want).abs().max()), float((loc - want_loc).abs().max()), float((w - want_w).abs().max())
        print(f"FIG N{n} {mask_kind} {tok} one launch vs three: out={err:.2e} (tol {tol:.2e}) loc={lerr:.2e} weights={werr:.2e}")
        assert bool(torch.isfinite(out).all()) and err <= tol and werr <= 1e-6
        assert lerr <= 1e-6 * max(1.0, float(want_loc.abs().max()))


def test_six_cameras_through_the_rig_entry_are_the_old_entry_bit_for_bit():
    """Six cameras launch the very kernels simpb_dfa_fused_forward[_cams] launch: the same bits from the three entries."""
    from simpb_amd import _lib as L
    from simpb_amd.plugin.ops import _ptr as P, _stream
    lib = L.lib()
    c = T.b_case("scene", "random")
    bs, a, n = c["bs"], c["A"], 6
    ss, st, anchor, learn, fix, proj, wh, fl, cl = (T.dev(c[k]).contiguous() for k in ("ss", "st", "anchor", "learn", "fix", "proj", "wh", "fl", "cl"))
    for f16 in (0, 1):
        feat = T.dev(c["col"], torch.float16 if f16 else torch.float32).contiguous()
        for mask in (None, T.dev(T.DROP)):
            got = []
            for entry in ("simpb_dfa_fused_forward_rig", "simpb_dfa_fused_forward_cams") + (("simpb_dfa_fused_forward",) if mask is None else ()):
                out = torch.full((bs, a, 256), float("nan"), device="cuda")
                loc = torch.full((bs, a, K.NPTS, n, 2), float("nan"), device="cuda")
                w = torch.full((bs, a, K.NPTS, n, K.LVL, K.GRP), float("nan"), device="cuda")
                tail = () if entry == "simpb_dfa_fused_forward" else (P(mask) if mask is not None else None,)
                L.check(getattr(lib, entry)(P(out), P(feat), f16, P(ss), P(st), P(anchor), P(learn), P(fix), P(proj), P(wh), P(fl), P(cl),
                                            P(loc), P(w), bs, n, feat.shape[1], 256, K.LVL, a, K.NFIX, K.NLEARN, K.GRP, *tail, _stream()),
                        entry)
                torch.cuda.synchronize()
                got.append((out, loc, w))
            for other in got[1:]:
                for s, t in zip(got[0], other):
                    assert torch.equal(s, t), (f16, mask is not None)
            assert bool(torch.isfinite(got[0][0]).all())
