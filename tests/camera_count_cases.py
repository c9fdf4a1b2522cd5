"""Inputs of the camera-count tests (tests/test_camera_count_host.py on the CPU, tests/test_gpu_camera_count_*.py on the GPU):
the operator cases of tests/test_samplers_float64.py section B at N cameras, and the small golden head on an N-camera ring.
No GPU and no product kernel here: numpy, simpb_amd.synth and the float64 statement tests/sampler_ref.py."""
import functools

import numpy as np

from tests import sampler_ref as S
from tests import test_samplers_float64 as T

OPS_CAMS = (1, 2, 3, 4, 5, 7, 8)                 # the fused launch alone (six is the shipped rig: its own tests)
HEAD_CAMS = (1, 5, 8)                            # the head against the oracle
SEED_CAMS = (1, 2, 3, 4, 5, 7, 8)                     # rigs whose seeds the CPU test vouches for
OPS_CASES = [("affine", "random"), ("affine", "dominant"), ("scene", "random"), ("scene", "dominant")]
MASKS = ("none", "ones", "one_left")
LVL, NFIX, NLEARN, NPTS, GRP = T.LVL, T.NFIX, T.NLEARN, T.NPTS, T.GRP
LPG = LVL * NPTS * GRP
BS, A = 3, 48
# anchors of the "scene" family per camera count, chosen on the CPU (test_camera_count_host.py::test_operator_cases_...): at
# most 2 % of the anchors carry a sample whose gate the fp32 error could flip
SCENE_SEED = {1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 7: 3, 8: 3}


def pyramids(n):
    """Camera sets of the N-camera operator case: the first ceil(N / 2) cameras on pyramid S1, the others on S2 (N = 1: S1)."""
    return [(p, k) for p, k in ((T.S1, (n + 1) // 2), (T.S2, n // 2)) if k]


def logits(rs, kind, n):
    scale = 2.0 if kind == "random" else 1.0
    fl = (rs.standard_normal((BS, A, LVL * NPTS, GRP)) * scale).astype(np.float32)
    cl = (rs.standard_normal((BS, n, LPG)) * 0.5).astype(np.float32)
    if kind == "dominant":    # one entry per group 30 above the rest
        hot = rs.randint(0, LVL * NPTS, (BS, A, GRP))
        np.put_along_axis(fl, hot[:, :, None, :], 30.0, axis=2)
    return fl.reshape(BS, A, LPG), cl


def mask_of(kind, n):
    """None, all ones, or one camera left per stream (another camera in every stream; N = 1: that one camera)."""
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones((BS, n), np.uint8)
    m = np.zeros((BS, n), np.uint8)
    for b in range(BS):
        m[b, (1 + b * max(1, n // 3)) % n] = 1
    return m


@functools.lru_cache(maxsize=None)
def ops_case(n, family, kind):
    """b_case of tests/test_samplers_float64.py ("affine" / "scene") with n cameras."""
    rs = np.random.RandomState(1000 * n + 5 + len(family) + 3 * len(kind))
    if family == "affine":      # non-zero fix_scale, learnable offsets and yaw; power-of-two image sizes
        anchor = np.zeros((BS, A, 11), np.float32)
        anchor[..., :2] = rs.standard_normal((BS, A, 2)) * 2
        anchor[..., 2] = rs.uniform(2, 10, (BS, A))
        anchor[..., 3:6] = rs.standard_normal((BS, A, 3)) * 0.3
        yaw = rs.uniform(-np.pi, np.pi, (BS, A))
        anchor[..., 6], anchor[..., 7] = np.sin(yaw), np.cos(yaw)
        proj = np.zeros((BS, n, 4, 4), np.float32)
        for cam in range(n):
            f = 28.0 + 2 * cam
            proj[:, cam, :3] = [[f, 0.5, 32.0, 1.0 - cam], [-0.25, f / 2, 16.0, 0.5 * cam], [0.01, -0.02, 1.0, 0.25 * cam]]
        proj[:, :, 3, 3] = 1.0
        wh = np.tile(np.array([64.0, 32.0], np.float32), (BS, n, 1))
        fix = rs.uniform(-0.5, 0.5, (NFIX, 3)).astype(np.float32)
    else:                          # the synthetic scene: an n-camera ring, anchors around the ego vehicle
        from simpb_amd import synth
        metas = synth.frame_metas(BS, 0, num_cams=n)
        proj, wh = metas["projection_mat"].numpy().astype(np.float32), metas["image_wh"].numpy().astype(np.float32)
        anchor = np.stack([synth.anchors(A, seed=SCENE_SEED[n] + b) for b in range(BS)]).astype(np.float32)
        anchor[..., :2] *= 0.5     # more key points inside the images
        fix = T.FIX_SCALE
    learn = rs.standard_normal((BS, A, NLEARN * 3)).astype(np.float32)
    groups = [T.make_maps(rs, "random", BS, k, 256, p) for p, k in pyramids(n)]
    col, ss, st = T.format_maps(groups)
    fl, cl = logits(rs, kind, n)
    c = dict(col=col, ss=ss, st=st, anchor=anchor, learn=learn, fix=fix, proj=proj, wh=wh, fl=fl, cl=cl, bs=BS, A=A, n=n)
    c["points"] = S.dfa_points(anchor, learn, fix, proj, wh)
    return c


def masked_points(c, mask):
    return c["points"] if mask is None else S.dfa_points(c["anchor"], c["learn"], c["fix"], c["proj"], c["wh"], mask)


def anchors_left_out(pts, mask):
    """Anchors with a sample of a valid camera whose gate the fp32 error of the projection could flip."""
    off = np.zeros(pts["loc"].shape[:1] + pts["loc"].shape[3:4], bool) if mask is None else mask == 0
    und = T.undecided(pts) & ~off[:, None, None, :]
    return und, int(und.any(axis=(2, 3)).sum())


def reference(c, tokens, loc32, w32, mask):
    """sampler_ref.daf on the kernel's own operands; a masked stream is evaluated with its masked cameras removed."""
    return T.b_reference(c, tokens, loc32, w32, np.ones((c["bs"], c["n"]), bool) if mask is None else mask != 0)


# ------------------------------------------------------------------------------------------------- the head on an N-camera ring
HEAD_BS, HEAD_FRAMES, HEAD_CAPACITY = 2, 3, 128
# weights, and feature maps per camera count, chosen on the CPU (test_camera_count_host.py::test_oracle_on_the_ring_...): of
# feature seeds 9..15 the one whose smallest ranking-cut gap over the streams and frames is the largest (all >= 5e-4)
WEIGHT_SEED, FEATURE_SEED = 5, {1: 13, 2: 15, 3: 13, 4: 9, 5: 9, 7: 9, 8: 12}
NEAR = 1e-4                           # within NEAR of flipping on the oracle's own numbers


def head_spec():
    from tests.helpers import load_golden, spec_of
    return spec_of(load_golden("head_small.npz"))


def build_head(spec, n, device="cpu", seed=WEIGHT_SEED):
    """tests.helpers.build_product_head at n cameras."""
    from simpb_amd import configs, plugin, synth
    cfg = configs.simpb_plus(anchor=synth.anchors(spec["num_anchor"]), num_cams=n)["model"]["head"]
    cfg["instance_bank"]["num_anchor"] = spec["num_anchor"]
    cfg["instance_bank"]["num_temp_instances"] = spec["num_temp"]
    cfg["num_anchor"] = spec["num_anchor"]
    cfg["decoder"] = dict(type="SparseBox3DDecoder", num_output=spec["num_output"])
    head = plugin.build_head(cfg).eval()
    synth.load_procedural(head, seed=seed)
    return head.to(device)


def frame_inputs(spec, n, f):
    """(feature maps [bs, n, C, H, W] per level holding f16 numbers, metas) of frame f of the HEAD_BS streams."""
    from simpb_amd import synth
    maps = [m.half().float() for m in synth.feature_maps_nchw(HEAD_BS, f, spec["image_wh"], num_cams=n, seed=FEATURE_SEED[n])]
    return maps, synth.frame_metas(HEAD_BS, f, spec["image_wh"], num_cams=n)


def one_stream(metas, b):
    return dict(projection_mat=metas["projection_mat"][b:b + 1], image_wh=metas["image_wh"][b:b + 1],
                timestamp=metas["timestamp"][b:b + 1], img_metas=[metas["img_metas"][b]])


def margins(want, oracle, metas_b, spec, warm):
    """What could flip between two fp32 evaluations of one frame, on the oracle's own numbers: the gaps at the three ranking
    cuts (update: best A - T current instances by the first layer's max-class logit; cache: best T by confidence; decode:
    best num_output by score) and the distance in pixels of the nearest projected anchor centre to an image border (the
    allocation's inside / outside test), over the learned anchors and every layer's refined set."""
    import torch
    out = {}
    bank = oracle.bank
    if warm:
        v = torch.sort(want["classification"][0].max(dim=-1).values.flatten(), descending=True).values
        k = bank.num_anchor - bank.num_temp
        out["update"] = float(v[k - 1] - v[k])
    c = torch.sort(bank.temp_confidence.flatten(), descending=True).values
    out["cache"] = float(c[bank.num_temp - 1] - c[bank.num_temp])
    s = torch.sort(want["classification"][-1][0].sigmoid().max(dim=-1).values, descending=True).values
    out["decode"] = float(s[spec["num_output"] - 1] - s[spec["num_output"]])
    proj, (w, h) = metas_b["projection_mat"][0].double(), spec["image_wh"]
    best = float("inf")
    for anc in [oracle.p["instance_bank.anchor"][None]] + list(want["prediction"]):
        x = anc[0].double()
        p = torch.einsum("cij,aj->aci", proj, torch.cat([x[:, :3], x.new_ones(len(x), 1)], 1))
        u, v_ = p[..., 0] / p[..., 2].clamp(min=1e-5), p[..., 1] / p[..., 2].clamp(min=1e-5)
        best = min(best, float(torch.stack([u.abs(), (u - w).abs(), v_.abs(), (v_ - h).abs()], -1).min()))
    out["border_px"] = best
    return out
