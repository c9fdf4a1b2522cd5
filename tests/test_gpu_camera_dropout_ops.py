"""GPU: the six `_cams` entry points (csrc/alloc.hip, csrc/dfa_prep.hip, csrc/deform_agg_fused.hip) through ctypes. The
comparators are the EXISTING entry points: for the allocation, on matrices that put every point of a masked camera outside
its image; for the aggregation, per stream at bs = 1 on the arrays compacted to the valid cameras -- "the frame as the
reference decodes it when given the remaining cameras only". What a masked camera's rows hold (NaN here) is never read."""
import functools

import numpy as np
import pytest
import torch

from simpb_amd import synth

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lib():
    from simpb_amd import _lib as L
    from simpb_amd.plugin.ops import _ptr, _stream
    return L, L.lib(), _ptr, _stream


def _u8(mask):
    return torch.tensor(mask, dtype=torch.uint8, device="cuda").contiguous()


def _opt(P, t):
    return P(t) if t is not None else None


# ---------------------------------------------------------------------------------------------------------------- allocation
BS, A, CAMS, PER_STREAM, IMG = 3, 48, 6, 128, (704.0, 256.0)
MASKS = [(1, 0, 1, 1, 1, 1), (1, 1, 1, 1, 1, 1), (0, 1, 1, 1, 1, 0)]
LIMITS = (35.0, 35.0, 10.0)
# every projected point lands at x = y = -1e5 with depth -1: flag 0 for every anchor
OUTSIDE = torch.tensor([[0.0, 0, 0, -1], [0, 0, 0, -1], [0, 0, 0, -1], [0, 0, 0, 1]])
TABLES = ("count", "group_start", "overflow", "pts", "d2", "q2a", "ctr", "a2q", "cam")


@functools.lru_cache(maxsize=None)
def _alloc_inputs():
    g = torch.Generator().manual_seed(2)
    anchor = torch.from_numpy(synth.anchors(A)).float()[None].repeat(BS, 1, 1)
    anchor[..., :2] += torch.randn(BS, A, 2, generator=g) * 3.0
    proj = synth.frame_metas(BS, 0)["projection_mat"].contiguous()
    masked, outside = proj.clone(), proj.clone()
    for b, row in enumerate(MASKS):
        for c, on in enumerate(row):
            if not on:
                masked[b, c], outside[b, c] = NAN, OUTSIDE
    return anchor.cuda(), proj.cuda(), masked.cuda(), outside.cuda()


def _alloc(form, anchor, proj, cam_valid=None, active=None, entry="cams", per_stream=PER_STREAM):
    """One allocation in the given form; entry: "cams" (the new entry points) or "old" (the existing ones). Returns every
    table on the host."""
    L, lib, P, S = _lib()
    bs, dev = anchor.shape[0], "cuda"
    ragged = form == "ragged"
    slots, rows = (bs * per_stream, 1) if ragged else (2 * per_stream, bs)
    groups = bs * CAMS if ragged else CAMS
    o = dict(flag=torch.full((bs, CAMS, A), 9, dtype=torch.uint8, device=dev), sel=torch.full((bs, CAMS, A, 2), -5.0, device=dev),
             depth=torch.full((bs, CAMS, A), -5.0, device=dev), count=torch.full((bs, CAMS), -5, dtype=torch.int32, device=dev),
             order=torch.zeros(bs, CAMS, A, dtype=torch.int32, device=dev),
             group_start=torch.full((groups + 1,), -5, dtype=torch.int32, device=dev),
             overflow=torch.full((1,), -5, dtype=torch.int32, device=dev), pts=torch.full((rows, slots, 2), -5.0, device=dev),
             d2=torch.full((rows, slots), -5.0, device=dev), q2a=torch.full((rows, slots), -5, dtype=torch.int32, device=dev),
             ctr=torch.full((rows, slots), -5, dtype=torch.int32, device=dev),
             a2q=torch.full((bs, A, CAMS), -5, dtype=torch.int32, device=dev), cam=torch.full((slots,), -5, dtype=torch.int32, device=dev))
    all15 = [P(o[k]) for k in ("flag", "sel", "depth", "count", "order", "group_start", "overflow", "pts", "d2", "q2a", "ctr", "a2q", "cam")]
    tail = [P(anchor), P(proj), bs, A, CAMS]
    cv, st = _opt(P, cam_valid), S()
    if ragged:
        args = all15 + tail + [per_stream, *IMG, *LIMITS]
        if entry == "cams":
            L.check(lib.simpb_alloc_ragged_cams(*args, _opt(P, active), cv, st), "alloc_ragged_cams")
        else:
            L.check(lib.simpb_alloc_ragged_active(*args, _opt(P, active), st), "alloc_ragged_active")
    elif form == "static":
        args = all15 + tail + [slots, *IMG, *LIMITS]
        if entry == "cams":
            L.check(lib.simpb_alloc_static_cams(*args, cv, st), "alloc_static_cams")
        else:
            L.check(lib.simpb_alloc_static(*args, st), "alloc_static")
    else:   # stepwise: project, compact, group table, scatter
        args = [P(o["flag"]), P(o["sel"]), P(o["depth"])] + tail + [*IMG, *LIMITS]
        if entry == "cams":
            L.check(lib.simpb_alloc_project_cams(*args, cv, st), "alloc_project_cams")
        else:
            L.check(lib.simpb_alloc_project(*args, st), "alloc_project")
        L.check(lib.simpb_alloc_compact(P(o["count"]), P(o["order"]), P(o["flag"]), bs, A, CAMS, st), "alloc_compact")
        L.check(lib.simpb_alloc_group_start(P(o["group_start"]), P(o["overflow"]), P(o["count"]), bs, CAMS, slots, st), "group_start")
        L.check(lib.simpb_alloc_scatter(P(o["pts"]), P(o["d2"]), P(o["q2a"]), P(o["ctr"]), P(o["a2q"]), P(o["cam"]), P(o["group_start"]),
                                        P(o["count"]), P(o["order"]), P(o["flag"]), P(o["sel"]), P(o["depth"]), bs, A, CAMS, slots,
                                        *IMG, st), "alloc_scatter")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _assert_same_tables(got, want, names=TABLES):
    for k in names:
        assert np.array_equal(got[k], want[k]), k
    for b in range(BS):   # order is defined up to the count
        for c in range(CAMS):
            n = int(want["count"][b, c])
            assert np.array_equal(got["order"][b, c, :n], want["order"][b, c, :n]), (b, c)


@pytest.mark.parametrize("form,active", [("static", None), ("stepwise", None), ("ragged", None), ("ragged", (1, 0, 1))],
                         ids=["static", "stepwise", "ragged", "ragged_with_a_paused_stream"])
def test_masked_camera_is_an_empty_group_of_the_allocation(form, active):
    anchor, proj, masked, outside = _alloc_inputs()
    act = _u8(active) if active is not None else None
    got = _alloc(form, anchor, masked, cam_valid=_u8(MASKS), active=act)
    want = _alloc(form, anchor, outside, active=act, entry="old")
    _assert_same_tables(got, want)
    full = _alloc(form, anchor, proj, active=act, entry="old")
    assert int(got["overflow"][0]) == 0 and int(got["count"].sum()) > 0
    for b, row in enumerate(MASKS):
        on = active is None or active[b]
        for c, valid in enumerate(row):
            if not valid or not on:   # flag 0, count 0, a2q = -1: an all-false column of the reference's trans_mask
                assert int(got["count"][b, c]) == 0 and (got["flag"][b, c] == 0).all() and (got["a2q"][b, :, c] == -1).all()
            else:                     # a valid camera keeps what the full rig gives it
                assert int(got["count"][b, c]) == int(full["count"][b, c])
                assert np.array_equal(got["flag"][b, c], full["flag"][b, c])
    assert int(full["count"][0, 1]) > 0 and int(full["count"][2, 0]) > 0   # the masked cameras did see anchors
    assert np.isfinite(got["pts"]).all() and np.isfinite(got["d2"]).all()
    if form == "ragged":   # the groups behind a masked camera move down: live slots first
        gs = got["group_start"]
        assert (np.diff(gs) >= 0).all() and int(gs[BS * CAMS]) == int(got["count"].sum())
        assert gs[1] == gs[2] and (got["cam"][:int(gs[BS * CAMS])] != 1).all()


@pytest.mark.parametrize("form", ["static", "stepwise", "ragged"])
def test_all_ones_mask_is_the_allocation_without_a_mask(form):
    anchor, proj, _, _ = _alloc_inputs()
    ones = _u8([[1] * CAMS] * BS)
    a = _alloc(form, anchor, proj, cam_valid=ones)
    b = _alloc(form, anchor, proj, cam_valid=None)
    c = _alloc(form, anchor, proj, entry="old")
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k


def test_a_masked_camera_cannot_raise_overflow():
    """Every stream loses its busiest camera; the capacity is what the largest remaining set needs: the full rig overflows
    it, the masked rig fills it exactly."""
    anchor, proj, _, _ = _alloc_inputs()
    need = _alloc("ragged", anchor, proj, entry="old")["count"]
    busiest = need.argmax(axis=1)
    rest = need.sum(axis=1) - need.max(axis=1)
    per_stream = int(rest.max())
    assert need.max(axis=1).min() > 0 and per_stream > 0, need
    rows = [[int(c != busiest[b]) for c in range(CAMS)] for b in range(BS)]
    assert int(_alloc("ragged", anchor, proj, cam_valid=_u8([[1] * CAMS] * BS), per_stream=per_stream)["overflow"][0]) == 1
    got = _alloc("ragged", anchor, proj, cam_valid=_u8(rows), per_stream=per_stream)
    assert int(got["overflow"][0]) == 0
    assert np.array_equal(got["count"].sum(axis=1), rest) and int(got["group_start"][BS * CAMS]) == int(rest.sum())


# --------------------------------------------------------------------------------------------------------------- aggregation
DBS, DA, WH = 2, 77, (352, 128)
L_, P_, G_, C_, FIX, LEARN = 4, 13, 8, 256, 7, 6
DROPPED = [(2,), (0, 5)]


@functools.lru_cache(maxsize=None)
def _dfa_inputs():
    """Operands of the shipped layout at the shapes of tests/test_gpu_ops.py::test_dfa_fused_launch_equals_three_launches,
    as the module computes them in front of the launch; `nan`: the same with everything of the masked cameras NaN."""
    from simpb_amd import configs, plugin
    from simpb_amd.plugin import ops
    cfg = configs.simpb_plus(anchor=synth.anchors(900))["model"]["head"]["deformable_model"]
    dfa = plugin.build_from_cfg(cfg, plugin.ATTENTION).eval()
    synth.load_procedural(dfa, seed=2)
    fm = ops.feature_maps_format([x.cuda() for x in synth.feature_maps_nchw(DBS, 0, WH)])
    tokens = fm[0].half().float().contiguous()          # f16 numbers, as the fp16 backbone leaves them
    ss, start = fm[1].int().contiguous(), fm[2].int().contiguous()
    feat = torch.from_numpy(synth.randn("dfa.feat", (DBS, DA, 256)))
    emb = torch.from_numpy(synth.randn("dfa.emb", (DBS, DA, 256)))
    anchor = torch.from_numpy(synth.anchors(DA, seed=4))[None].repeat(DBS, 1, 1)
    anchor[..., :2] *= 0.5   # more key points inside the images
    metas = synth.frame_metas(DBS, 0, WH)
    proj, wh = metas["projection_mat"].float().contiguous(), metas["image_wh"].float().contiguous()
    with torch.no_grad():
        learn = dfa.kps_generator.learnable_fc(feat).contiguous()
        feat_logits = dfa.weights_fc(feat + emb).contiguous()
        cam_embed = dfa.camera_encoder(proj[:, :, :3].reshape(DBS, 6, -1))
        cam_logits = torch.nn.functional.linear(cam_embed, dfa.weights_fc.weight).contiguous()
    x = dict(tokens=tokens, ss=ss, start=start, anchor=anchor.cuda(), learn=learn.cuda(), fix=dfa.kps_generator.fix_scale.detach().float().cuda().contiguous(),
             proj=proj.cuda(), wh=wh.cuda(), feat_logits=feat_logits.cuda(), cam_logits=cam_logits.cuda())
    nan = dict(x, tokens=tokens.clone(), proj=x["proj"].clone(), wh=x["wh"].clone(), cam_logits=x["cam_logits"].clone())
    per_cam = tokens.shape[1] // 6
    assert int(start[1, 0]) == per_cam
    for b, drop in enumerate(DROPPED):
        for c in drop:
            nan["tokens"][b, c * per_cam:(c + 1) * per_cam] = NAN
            nan["proj"][b, c], nan["wh"][b, c], nan["cam_logits"][b, c] = NAN, NAN, NAN
    return x, nan


def _fused(x, cam_valid, f16):
    L, lib, P, S = _lib()
    tokens = x["tokens"].half().contiguous() if f16 else x["tokens"]
    bs = tokens.shape[0]
    out = torch.full((bs, DA, C_), NAN, device="cuda")
    loc = torch.full((bs, DA, P_, 6, 2), NAN, device="cuda")
    w = torch.full((bs, DA, P_, 6, L_, G_), NAN, device="cuda")
    L.check(lib.simpb_dfa_fused_forward_cams(
        P(out), P(tokens), 1 if f16 else 0, P(x["ss"]), P(x["start"]), P(x["anchor"]), P(x["learn"]), P(x["fix"]), P(x["proj"]),
        P(x["wh"]), P(x["feat_logits"]), P(x["cam_logits"]), P(loc), P(w), bs, 6, tokens.shape[1], C_, L_, DA, FIX, LEARN, G_,
        _opt(P, cam_valid), S()), "dfa_fused_forward_cams")
    torch.cuda.synchronize()
    return out, loc, w


def _three(x, cam_valid=None, entry="cams", rows=None, cams=None):
    """points + weights + the drop-in aggregation operator; rows=b, cams=[...]: stream b alone on the compacted arrays,
    through the existing entry points."""
    L, lib, P, S = _lib()
    sel = lambda t, cam_dim=True: t if rows is None else (t[rows:rows + 1][:, cams] if cam_dim else t[rows:rows + 1]).contiguous()  # noqa: E731
    proj, wh, cl = sel(x["proj"]), sel(x["wh"]), sel(x["cam_logits"])
    anchor, learn, fl, tokens = (sel(x[k], False) for k in ("anchor", "learn", "feat_logits", "tokens"))
    ss, start = (x["ss"], x["start"]) if rows is None else (x["ss"][cams].contiguous(), x["start"][cams].contiguous())
    bs, nc = anchor.shape[0], proj.shape[1]
    loc = torch.full((bs, DA, P_, nc, 2), NAN, device="cuda")
    w = torch.full((bs, DA, P_, nc, L_, G_), NAN, device="cuda")
    out = torch.full((bs, DA, C_), NAN, device="cuda")
    if entry == "cams":
        cv = _opt(P, cam_valid)
        L.check(lib.simpb_dfa_points_cams(P(loc), None, P(anchor), P(learn), P(x["fix"]), P(proj), P(wh), bs, DA, FIX, LEARN, nc, cv, S()),
                "dfa_points_cams")
        L.check(lib.simpb_dfa_weights_cams(P(w), P(fl), P(cl), bs, DA, nc, L_, P_, G_, cv, S()), "dfa_weights_cams")
    else:
        L.check(lib.simpb_dfa_points(P(loc), None, P(anchor), P(learn), P(x["fix"]), P(proj), P(wh), bs, DA, FIX, LEARN, nc, S()), "dfa_points")
        L.check(lib.simpb_dfa_weights(P(w), P(fl), P(cl), bs, DA, nc, L_, P_, G_, S()), "dfa_weights")
    L.check(lib.simpb_deformable_aggregation_forward(P(out), P(tokens), P(ss), P(start), P(loc), P(w), bs, nc, tokens.shape[1], C_, L_, DA,
                                                     P_, G_, S()), "deformable_aggregation_forward")
    torch.cuda.synchronize()
    return out, loc, w


@functools.lru_cache(maxsize=None)
def _subset_reference():
    """Per stream: the existing three launches at bs = 1 on the arrays compacted to the valid cameras (the token array
    stays as it is: NaN blocks and all). Computed once."""
    _, nan = _dfa_inputs()
    ref = []
    for b, drop in enumerate(DROPPED):
        kept = [c for c in range(6) if c not in drop]
        ref.append((kept,) + _three(nan, entry="old", rows=b, cams=kept))
    return ref


def _mask():
    return _u8([[int(c not in drop) for c in range(6)] for drop in DROPPED])


def _check_against_subset(out, loc, w):
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(loc).all()) and bool(torch.isfinite(w).all())
    for b, (kept, want_out, want_loc, want_w) in enumerate(_subset_reference()):
        for c in DROPPED[b]:
            assert bool((w[b, :, :, c] == 0.0).all()) and bool((loc[b, :, :, c] == -1.0).all()), (b, c)
        valid = ((want_loc > 0) & (want_loc < 1)).all(-1)
        assert int(valid.sum()) > 100
        assert float((w[b][:, :, kept] - want_w[0]).abs().max()) <= 1e-6, b
        assert float((loc[b][:, :, kept] - want_loc[0]).abs().max()) <= 1e-6 * max(1.0, float(want_loc.abs().max())), b
        assert float((w[b].sum(dim=(1, 2, 3)) - 1.0).abs().max()) <= 1e-5     # renormalised over the valid cameras
        assert float((out[b] - want_out[0]).abs().max()) <= 2e-5 * max(1.0, float(want_out.abs().max())), b


@pytest.mark.parametrize("f16", [False, True], ids=["f32_tokens", "f16_tokens"])
def test_fused_aggregation_without_the_masked_cameras_equals_the_subset(f16):
    _, nan = _dfa_inputs()
    _check_against_subset(*_fused(nan, _mask(), f16))


def test_three_launch_aggregation_without_the_masked_cameras_equals_the_subset():
    _, nan = _dfa_inputs()
    _check_against_subset(*_three(nan, _mask()))


def test_all_ones_mask_is_the_aggregation_without_a_mask():
    x, _ = _dfa_inputs()
    ones = _u8([[1] * 6] * DBS)
    for f16 in (False, True):
        a, b = _fused(x, ones, f16), _fused(x, None, f16)
        for s, t in zip(a, b):
            assert torch.equal(s, t), f16
    L, lib, P, S = _lib()
    out = torch.full((DBS, DA, C_), NAN, device="cuda")   # ... and NULL is the entry point without the argument
    L.check(lib.simpb_dfa_fused_forward(P(out), P(x["tokens"]), 0, P(x["ss"]), P(x["start"]), P(x["anchor"]), P(x["learn"]), P(x["fix"]),
                                        P(x["proj"]), P(x["wh"]), P(x["feat_logits"]), P(x["cam_logits"]), None, None, DBS, 6,
                                        x["tokens"].shape[1], C_, L_, DA, FIX, LEARN, G_, S()), "dfa_fused_forward")
    torch.cuda.synchronize()
    assert torch.equal(out, _fused(x, None, False)[0])
    a, b, c = _three(x, ones), _three(x, None), _three(x, entry="old")
    for s, t, u in zip(a, b, c):
        assert torch.equal(s, t) and torch.equal(s, u)


def test_a_stream_without_any_valid_camera_gives_zeros():
    """Refused on the host (runner.normalise_cameras); in the kernels it is finite all the same: no weight, no tap, zeros
    out -- not 0 x NaN and no division by the zero sum. Stream 0 keeps its cameras and its result."""
    _, nan = _dfa_inputs()
    every = dict(nan, tokens=nan["tokens"].clone(), proj=nan["proj"].clone(), wh=nan["wh"].clone(), cam_logits=nan["cam_logits"].clone())
    every["tokens"][1], every["proj"][1], every["wh"][1], every["cam_logits"][1] = NAN, NAN, NAN, NAN
    mask = _u8([[int(c not in DROPPED[0]) for c in range(6)], [0] * 6])
    _, want_out, _, _ = _subset_reference()[0]
    for out, loc, w in (_fused(every, mask, False), _fused(every, mask, True), _three(every, mask)):
        assert bool((out[1] == 0).all()) and bool((w[1] == 0).all()) and bool((loc[1] == -1).all())
        assert float((out[0] - want_out[0]).abs().max()) <= 2e-5 * max(1.0, float(want_out.abs().max()))
