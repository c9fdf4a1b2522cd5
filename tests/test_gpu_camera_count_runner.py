"""GPU: the frame runners on rigs of five, seven and eight cameras with a real backbone (ResNet50 + FPN in fp16 at 176 x 64,
a head of 128 anchors), graphs on -- a replayed frame holds f16 token rows only, which only the one-launch 3D aggregation
(csrc/deform_agg_fused.hip) reads.

(a) replayed frames equal the eager frames of a second runner on the same inputs, bit for bit (FrameRunner, PipelinedRunner);
(b) eight cameras, `cameras=` drops three of them in stream 1 of two: that stream equals the subset oracle
    (tests/camera_dropout_ref.py) on the five remaining, frame by frame from the state the batch held (the recipe of
    tests/test_gpu_camera_count_head.py, 1e-3); stream 0 equals its run without a mask bit for bit;
(c) a raw_rig of seven sources (two sizes, two formats, two resize rules): the ingest's image tensor equals the witnesses
    (tests/preprocess_ref.py), the 3D half equals the runner fed the witnesses' fp32 images, and every camera's 2D boxes come
    back in that camera's own source pixels;
(d) eight cameras with world_output: the row counts are those of results.format_sample, and a stream exported from one runner
    and adopted into a second eight-camera runner goes on bit for bit."""
import copy
import functools

import numpy as np
import pytest
import torch

from simpb_amd import preprocess as P
from simpb_amd import synth
from tests import camera_dropout_ref as C
from tests import camera_count_cases as K

pytestmark = pytest.mark.gpu

WH = (176, 64)
SPEC = dict(num_anchor=128, num_temp=64, num_output=32)
CAP = 256


@functools.lru_cache(maxsize=None)
def _pristine(n):
    """The small detector at n cameras (real ResNet50 + FPN, fp16 backbone; the head of SPEC), built once and never run: every
    runner gets its own deep copy."""
    from simpb_amd import configs, plugin
    cfg = configs.simpb_plus(anchor=synth.anchors(SPEC["num_anchor"]), num_cams=n)
    h = cfg["model"]["head"]
    h["instance_bank"]["num_anchor"] = h["num_anchor"] = SPEC["num_anchor"]
    h["instance_bank"]["num_temp_instances"] = SPEC["num_temp"]
    h["decoder"] = dict(type="SparseBox3DDecoder", num_output=SPEC["num_output"])
    model = plugin.build_detector(cfg["model"]).eval()
    synth.load_procedural(model)
    model.cuda()
    model.fuse_conv_bn()
    model.half_backbone()
    return model


def _runner(kind, n, bs, use_graph=True, **kw):
    from simpb_amd import runner as RN
    cls = dict(plain=RN.FrameRunner, pipe=RN.PipelinedRunner)[kind]
    return cls(copy.deepcopy(_pristine(n)), bs, (WH[1], WH[0]), capacity=CAP, device=torch.device("cuda"), use_graph=use_graph,
               independent_streams=bs > 1, **kw)


def _same_bytes(a, b):
    a, b = torch.as_tensor(np.asarray(a)) if not torch.is_tensor(a) else a, torch.as_tensor(np.asarray(b)) if not torch.is_tensor(b) else b
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _drive(r, frames, feed, metas, **step_kw):
    """`frames` steps; per frame (results, rec3d, rec2d), a pipelined runner's one-frame delay undone."""
    got = []
    for f in range(frames):
        res = r.step(feed(f), metas(f), **{k: v(f) for k, v in step_kw.items()})
        if res is not None:
            got.append((res, r.last_rec3d.clone(), r.last_rec2d.clone()))
    if hasattr(r, "flush"):
        got.append((r.flush(), r.last_rec3d.clone(), r.last_rec2d.clone()))
    assert len(got) == frames and r.stats["overflow"] == 0, r.stats
    return got


def _assert_streams_equal(a, b, what, streams=None, skip=()):
    for f, ((ra, a3, a2), (rb, b3, b2)) in enumerate(zip(a, b)):
        for s in (range(a3.shape[0]) if streams is None else streams):
            assert _same_bytes(a3[s], b3[s]), (what, f, s, "rec3d")
            assert bool(torch.isfinite(a3[s][..., :13]).all()), (what, f, s)
            if streams is None:
                assert _same_bytes(a2[s], b2[s]), (what, f, s, "rec2d")
            xa, xb = ra[s]["img_bbox"], rb[s]["img_bbox"]
            assert xa.keys() == xb.keys()
            for k in xa:
                if k in skip:
                    continue
                if k == "world":
                    assert xa[k]["count"] == xb[k]["count"] and _same_bytes(xa[k]["record"], xb[k]["record"]), (what, f, s, k)
                elif torch.is_tensor(xa[k]) or isinstance(xa[k], np.ndarray):
                    assert _same_bytes(xa[k], xb[k]), (what, f, s, k)
                else:
                    assert np.array_equal(np.asarray(xa[k]), np.asarray(xb[k])), (what, f, s, k)


# ------------------------------------------------------------------------------------------------ (a) replayed = eager frames
# FrameRunner replays from its third frame on, a pipelined runner from the fifth (one graph per feature slot)
@pytest.mark.parametrize("kind,frames", [("plain", 5), ("pipe", 7)])
@pytest.mark.parametrize("n", [5, 8])
def test_replayed_frames_equal_eager_frames(n, kind, frames):
    bs = 2
    feed = lambda f: synth.images(bs, f, WH, num_cams=n).cuda()          # noqa: E731
    metas = lambda f: synth.frame_metas(bs, f, WH, num_cams=n)           # noqa: E731
    eager = _runner(kind, n, bs, use_graph=False)
    a = _drive(eager, frames, feed, metas)
    graph = _runner(kind, n, bs, use_graph=True)
    b = _drive(graph, frames, feed, metas)
    print(f"FIG N{n} {kind} eager {eager.stats} replayed {graph.stats}")
    assert eager.stats["replay"] == 0 and graph.stats["replay"] >= 3, (eager.stats, graph.stats)
    _assert_streams_equal(a, b, (n, kind))
    groups = [hi - lo for lo, hi in a[-1][0][0]["img_bbox"]["query_groups"]]
    assert len(groups) == n and sum(groups) > 0, groups


# ------------------------------------------------------------------------- (b) three of eight cameras dropped in one stream
KEPT = (0, 1, 3, 4, 6)


def _maps_of(col, shapes, n):
    """[bs, n, C, H, W] per level from the token buffer [bs, n * tokens, C] of ops.feature_maps_format's layout."""
    bs, _, c = col.shape
    per = col.reshape(bs, n, -1, c)
    out, start = [], 0
    for h, w in shapes:
        out.append(per[:, :, start:start + h * w].reshape(bs, n, h, w, c).permute(0, 1, 4, 2, 3).contiguous())
        start += h * w
    assert start == per.shape[2]
    return out


def test_three_of_eight_cameras_dropped_in_one_stream(monkeypatch):
    from oracle import simpb_ref as R
    n, bs, frames = 8, 2, 4
    feed = lambda f: synth.images(bs, f, WH, num_cams=n).cuda()          # noqa: E731
    metas = lambda f: synth.frame_metas(bs, f, WH, num_cams=n)           # noqa: E731
    rows = C.mask_rows([tuple(range(n)), KEPT], n)
    plain = _drive(_runner("plain", n, bs), frames, feed, metas)
    r = _runner("plain", n, bs)
    head, bank = r.head, r.head.instance_bank
    params = {k: v.detach().cpu() for k, v in head.state_dict().items()}
    spec = dict(SPEC, image_wh=WH)
    extractor = copy.deepcopy(_pristine(n))
    masked, prev_metas = [], None
    for f in range(frames):
        m = metas(f)
        m["projection_mat"][1, [c for c in range(n) if c not in KEPT]] = float("nan")
        torch.cuda.synchronize()
        state = {k: v.clone().cpu() for k, v in bank._static.items()}
        res = r.step(feed(f), m, cameras=rows)
        masked.append((res, r.last_rec3d.clone(), r.last_rec2d.clone()))
        # the subset oracle of stream 1 on this frame's tokens (f16 numbers), from the state the batch held for it
        with torch.no_grad():
            fm = extractor.extract_feat(feed(f))
            col, shapes = fm[0].float().cpu(), [tuple(int(v) for v in hw) for hw in fm[1][0].tolist()]
        oracle = R.OracleHead(params, head.operation_order, SPEC["num_anchor"], SPEC["num_temp"], SPEC["num_output"])
        if f > 0:
            ob = oracle.bank
            ob.cached_feature, ob.cached_anchor = state["cached_feature"][1:2].clone(), state["cached_anchor"][1:2].clone()
            ob.confidence, ob.instance_id = state["confidence"][1:2].clone(), state["instance_id"][1:2].clone()
            ob.prev_id = int(state["prev_id"])
            ob.metas = dict(timestamp=prev_metas["timestamp"][1:2], img_metas=[prev_metas["img_metas"][1]])
        with torch.no_grad():
            want, _ = C.oracle_frame(monkeypatch, oracle, _maps_of(col, shapes, n), metas(f), KEPT, sample=1)
        margins = K.margins(want, oracle, K.one_stream(dict(metas(f), projection_mat=metas(f)["projection_mat"][:, list(KEPT)]), 1), spec, f > 0)
        want_res = oracle.post_process(want, K.one_stream(metas(f), 1))[0]
        got = res[1]["img_bbox"]
        a = torch.cat([got["boxes_3d"].float(), got["scores_3d"].float()[:, None]], 1)
        b = torch.cat([want_res["boxes_3d"], want_res["scores_3d"][:, None]], 1)
        d = torch.cdist(a.double(), b.double(), p=float("inf"))
        err = float(torch.maximum(d.min(dim=1).values, d.min(dim=0).values).max())
        cams2d = sorted(set(got["camidx_2d"].long().tolist()))
        print(f"FIG N8 dropped frame {f} stream 1: detections as row sets err={err:.2e} 2D cameras={cams2d} "
              f"2D boxes {len(got['boxes_2d'])} (oracle {len(want_res['boxes_2d'])}) oracle margins={ {k: f'{v:.1e}' for k, v in margins.items()} }")
        assert err <= 1e-3, (f, err)
        assert not set(cams2d) - set(KEPT) and len(got["boxes_2d"]) == len(want_res["boxes_2d"]), (f, cams2d)
        prev_metas = metas(f)
    assert r.cam_masked and r.stats["replay"] >= 2 and r.stats["overflow"] == 0, r.stats
    _assert_streams_equal(plain, masked, "stream 0 beside a masked stream", streams=[0])
    assert not _same_bytes(plain[1][1][1], masked[1][1][1])     # the mask is no small change to stream 1


# ------------------------------------------------------------------------------------------- (c) a raw rig of seven sources
NORM = P.IMG_NORM_CFG
WIDE = ((150, 400), "bgr", "jfif", dict(resize=0.44, crop=(0, 2, 176, 66)))
SMALL = ((120, 320), "nv12", "jfif", dict(resize=0.55, crop=(0, 2, 176, 66)))
RIG7 = (WIDE, SMALL, WIDE, SMALL, WIDE, SMALL, WIDE)


def _source(spec):
    hw, fmt, colour, aug = spec
    return P.CameraSource(hw, aug, fmt, colour)


@functools.lru_cache(maxsize=None)
def _picture(c, f):
    """Camera c's picture of frame f % 3: (its surface u8 [bytes], the BGR picture the surface holds)."""
    from tests import surface_ref as S
    from tests import yuv_ref as Y
    hw, fmt, colour, _ = RIG7[c]
    bgr = synth.raw_frames(1, f % 3, src_hw=hw, num_cams=7)[0, c].numpy()
    layout = _source(RIG7[c]).surface
    if fmt == "bgr":
        return torch.from_numpy(S.pack(bgr, layout, 0xEE)), bgr
    nv12 = Y.bgr_to_nv12(bgr, colour)
    return torch.from_numpy(S.pack(nv12, layout, 0xEE)), Y.yuv420sp_to_bgr(nv12, colour)


def test_raw_rig_of_seven_sources():
    from tests import preprocess_ref as R
    n, frames = 7, 4
    sources = [_source(s) for s in RIG7]
    handed = []

    def surfaces(f):
        row = [_picture(c, f)[0].cuda() for c in range(n)]
        handed.append(row)       # every surface stays referenced until the test ends
        return [list(row)]

    # the ingest alone: the image tensor equals the witnesses' operand, camera by camera
    rig = P.RigPlan(sources)
    got = rig.run_surfaces(surfaces(0)[0])
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, WH[1], WH[0], 4) and len(set(rig.src_rows)) == 2
    for c in range(n):
        want = torch.from_numpy(R.nhwc4_f16(_picture(c, 0)[1][None], RIG7[c][3], NORM))[0]
        assert _same_bytes(got[c].cpu(), want), ("witness", c)
    assert np.array_equal(rig.box2d_table()[:, 3], np.float32(1.0) / np.array([s[3]["resize"] for s in RIG7], np.float32))
    # the runner: the 3D half equals the runner fed the witnesses' fp32 images; 2D rows follow each camera's own rule
    fp32 = lambda f: torch.stack([torch.from_numpy(R.pipeline_nchw(_picture(c, f)[1], RIG7[c][3], NORM)) for c in range(n)])[None].cuda()  # noqa: E731
    r = _runner("plain", n, 1, raw_rig=sources)
    rig_run = _drive(r, frames, surfaces, lambda f: synth.frame_metas(1, f, WH, num_cams=n))
    assert r.stats["replay"] >= 2, r.stats
    runs = {}
    for rule, aug in (("wide", WIDE[3]), ("small", SMALL[3])):
        def metas(f, aug=aug):
            m = synth.frame_metas(1, f, WH, num_cams=n)
            m["img_metas"][0]["aug_config"] = dict(aug)
            return m
        ref = _runner("plain", n, 1)
        runs[rule] = _drive(ref, frames, fp32, metas)
        assert ref.stats == r.stats, (ref.stats, r.stats)
        _assert_streams_equal(runs[rule], rig_run, "3D half, rule " + rule, streams=[0], skip=("boxes_2d",))
    differ = boxes = 0
    for f in range(frames):
        g2, a2, b2 = rig_run[f][2][0], runs["wide"][f][2][0], runs["small"][f][2][0]
        cam = g2[:, 7]
        assert torch.equal(cam, a2[:, 7]) and torch.equal(cam, b2[:, 7])
        wide = (cam >= 0) & (cam.long() % 2 == 0)
        small = (cam >= 0) & (cam.long() % 2 == 1)
        assert torch.equal(g2[wide], a2[wide]) and torch.equal(g2[small], b2[small]), f
        differ += int((a2[small, :4] != b2[small, :4]).any())
        box, boxa, boxb = (x[f][0][0]["img_bbox"]["boxes_2d"] for x in (rig_run, runs["wide"], runs["small"]))
        odd = rig_run[f][0][0]["img_bbox"]["camidx_2d"].long() % 2 == 1
        assert torch.equal(box[~odd], boxa[~odd]) and torch.equal(box[odd], boxb[odd]), f
        boxes += len(box)
    print(f"FIG N7 raw rig: {boxes} 2D boxes over {frames} frames, frames where the two rules differ: {differ}")
    assert differ and boxes, "the two rules never gave different boxes: the comparison shows nothing"


# --------------------------------------------------------------------------- (d) world record and a stream that moves on
def _world_metas(n, bs):
    from tests import world_cases as W

    @functools.lru_cache(maxsize=None)
    def metas(f):
        m = synth.frame_metas(bs, f, WH, num_cams=n)
        rng = np.random.default_rng(700 + f)
        for s, im in enumerate(m["img_metas"]):
            im.update(W.random_pose(rng), token=f"s{s}-f{f}")
        return m
    return metas


def test_world_record_and_a_stream_adopted_by_a_second_eight_camera_runner():
    from simpb_amd import results
    from tests import world_cases as W
    n, bs, frames, move = 8, 2, 6, 3
    world = dict(classes=W.CLASSES, tracking=True, threshold=0.05)
    feed = lambda f: synth.images(bs, f, WH, num_cams=n).cuda()          # noqa: E731
    metas = _world_metas(n, bs)
    x, y = _runner("plain", n, bs, world_output=world), _runner("plain", n, bs, world_output=world)
    a, b, kept = [], [], 0
    for f in range(frames):
        res = x.step(feed(f), metas(f))
        a.append((res, x.last_rec3d.clone(), x.last_rec2d.clone()))
        for s in range(bs):     # the row counts are format_sample's
            det, info = res[s]["img_bbox"], metas(f)["img_metas"][s]
            w = det["world"]
            assert w["record"].shape == (w["count"], 16)
            want = results.format_sample(det, info, W.CLASSES, world["tracking"], world["threshold"])
            W.assert_same_annos(results.annos_from_world(w["record"], w["count"], info["token"], W.CLASSES, world["tracking"]),
                                want, world["tracking"])
            kept += w["count"]
        torch.cuda.synchronize()
        assert x.last_world_count.tolist() == [r_["img_bbox"]["world"]["count"] for r_ in res]
        state = x.export_stream(1) if f == move - 1 else None
        if state is not None:
            kept_state = state
        res = y.step(feed(f), metas(f), adopt={1: kept_state} if f == move else None)
        b.append((res, y.last_rec3d.clone(), y.last_rec2d.clone()))
    print(f"FIG N8 world rows kept={kept} of {frames * bs * SPEC['num_output']}; x {x.stats} y {y.stats}")
    assert 0 < kept < frames * bs * SPEC["num_output"]
    assert y.stats.get("adopt") == 1 and "adopt" not in x.stats and x.stats["replay"] >= 3 and x.stats["overflow"] == 0
    _assert_streams_equal(a, b, "adopted into the twin")
