"""GPU: camera dropout through the head and the three runners (SimPBHead metas["camera_valid"], step / launch `cameras=`).

1. Against the subset oracle (tests/camera_dropout_ref.py): the product head runs on all six cameras -- NaN tokens, NaN
   projection_mat and image_wh rows for the masked ones -- and the oracle on the kept cameras only. Weights, maps and bound
   are those of tests/test_gpu_head.py::test_head_vs_oracle_other_seed (head_small.npz spec, synth.load_procedural seed 5,
   feature maps seed 9, every output tensor within 1e-3, position by position). The oracle's own margins at the bank's two
   top-k cuts are measured on the CPU first, printed, and must be >= 1e-3 wherever they feed a compared output.
2. The runners on a small real backbone with raw u8 frames (800 x 300 -> 352 x 128), bs = 1: a masked camera's slot holds
   random bytes that change every frame and differ from run to run."""
import copy
import functools

import numpy as np
import pytest
import torch

from simpb_amd import synth
from tests import camera_dropout_ref as C
from tests.helpers import build_product_head, load_golden, metas_to, spec_of

pytestmark = pytest.mark.gpu

NAN = float("nan")
K5 = (0, 2, 3, 4, 5)
STREAM0 = [C.ALL, K5, K5, C.ALL]                          # a camera is lost for two frames and comes back
STREAM1 = [C.ALL, C.ALL, (0, 1, 2, 3, 4), (0, 1, 2, 3)]   # another stream loses one camera, then a second
KEYS = ("prediction", "classification", "quality", "prediction2d", "classification2d")


def _setup():
    from oracle import simpb_ref as R
    spec = spec_of(load_golden("head_small.npz"))
    head = build_product_head(spec)
    synth.load_procedural(head, seed=5)
    params = {k: v.detach().cpu() for k, v in head.state_dict().items()}
    make = lambda: R.OracleHead(params, head.operation_order, spec["num_anchor"], spec["num_temp"], spec["num_output"])  # noqa: E731
    return spec, head, make


def _frame(bs, f, wh):
    return synth.feature_maps_nchw(bs, f, wh, seed=9), synth.frame_metas(bs, f, wh)


def _oracle_sequence(monkeypatch, make, bs, wh, schedule, sample=None, what=""):
    """The whole sequence through one oracle on the CPU, before any GPU run; its margins printed and checked: the update cut
    of a warm frame feeds that frame's outputs, the cache cut of every frame but the last feeds the next frame's."""
    oracle, wants = make(), []
    with torch.no_grad():
        for f, kept in enumerate(schedule):
            maps, metas = _frame(bs, f, wh)
            want, cuts = C.oracle_frame(monkeypatch, oracle, maps, metas, kept, sample)
            print(f"oracle margins {what} frame {f} kept {kept}: update cut {cuts['update']}, cache cut {cuts['cache']}")
            feeding = [cuts["update"]] if f > 0 else []
            if f + 1 < len(schedule):
                feeding.append(cuts["cache"])
            assert all(m is not None and m >= 1e-3 for m in feeding), (what, f, cuts)
            wants.append(want)
    return wants


def _product_inputs(bs, f, wh, kept_rows):
    """The frame as the product gets it: all six cameras, everything of a masked camera NaN."""
    maps, metas = _frame(bs, f, wh)
    maps = [m.clone() for m in maps]
    metas = dict(metas, projection_mat=metas["projection_mat"].clone(), image_wh=metas["image_wh"].clone())
    for b, kept in enumerate(kept_rows):
        for c in range(6):
            if c not in kept:
                for m in maps:
                    m[b, c] = NAN
                metas["projection_mat"][b, c] = NAN
    return maps, metas


def _compare(got, want, what, rows=None, groups=None):
    """Every tensor of KEYS within 1e-3, shapes equal. rows = b: `got` is a batch, stream b of it is compared (its 2D rows
    are the slots of its own camera groups in the flat layout, per layer: groups[layer] = (lo, hi))."""
    for k in KEYS:
        for li, (a, w) in enumerate(zip(got[k], want[k])):
            if w is None:
                assert a is None, (what, k, li)
                continue
            if rows is not None:
                a = a[:, groups[li][0]:groups[li][1]] if k.endswith("2d") else a[rows:rows + 1]
            assert a.shape == w.shape, (what, k, li, a.shape, w.shape)
            err = float((a.cpu() - w).abs().max()) if w.numel() else 0.0
            assert err <= 1e-3, (what, k, li, err)


# ------------------------------------------------------------------------------------------------------ 1. subset oracle
def test_reference_batch_with_a_camera_lost_and_back_vs_subset_oracle(monkeypatch):
    """bs 2 in the reference's batch layout, dynamic capacity, the same mask for both samples. The bank carries across frames
    whose camera sets differ. (The bank after the last frame is not compared: its cut is 1.4e-4 in the oracle.)"""
    from simpb_amd.plugin import ops
    spec, head, make = _setup()
    wh, bs = spec["image_wh"], 2
    wants = _oracle_sequence(monkeypatch, make, bs, wh, STREAM0, what="batch")
    with torch.no_grad():
        for f, kept in enumerate(STREAM0):
            maps, metas = _product_inputs(bs, f, wh, [kept] * bs)
            dm = metas_to(metas, "cuda")
            dm["image_wh"][:, [c for c in range(6) if c not in kept]] = NAN
            if kept != C.ALL:
                dm["camera_valid"] = torch.tensor(C.mask_rows([kept] * bs), dtype=torch.uint8, device="cuda")
            got = head(ops.feature_maps_format([x.cuda() for x in maps]), dm)
            _compare(got, wants[f], ("batch", f))
            assert torch.equal(got["instance_id"].cpu(), wants[f]["instance_id"]), f
            n2 = [hi - lo for lo, hi in got["ref_query_groups_list"][-1]]
            assert len(n2) == 6 and all((n2[c] == 0) == (c not in kept) for c in range(6)), (f, n2)   # an empty camera group


class _Served(torch.nn.Module):
    def __init__(self, head):
        super().__init__()
        self.head, self.maps = head, None

    def extract_feat(self, img):
        return self.maps


def test_independent_streams_each_vs_its_own_subset_oracle(monkeypatch):
    """Static capacity, bs 2 as independent streams through FrameRunner (eager), each stream against its own batch-of-one
    oracle over the whole sequence. Fresh track ids are numbered through the batch (one counter), so a stream's ids equal
    its oracle's up to ONE relabelling that holds over all four frames; where an instance has no id (-1) is equal."""
    from simpb_amd.plugin import ops
    from simpb_amd.runner import FrameRunner
    spec, head, make = _setup()
    wh, bs, cap = spec["image_wh"], 2, 128
    schedules = [STREAM0, STREAM1]
    wants = [_oracle_sequence(monkeypatch, make, bs, wh, schedules[b], sample=b, what=f"stream {b}") for b in range(bs)]
    served = _Served(head)
    runner = FrameRunner(served, bs, (wh[1], wh[0]), capacity=cap, device=torch.device("cuda"), use_graph=False,
                         independent_streams=True)
    captured = {}
    head.register_forward_hook(lambda m, i, o: captured.update(outs=o))
    relabel = [dict(), dict()]
    with torch.no_grad():
        for f in range(len(STREAM0)):
            kept = [schedules[b][f] for b in range(bs)]
            maps, metas = _product_inputs(bs, f, wh, kept)
            served.maps = ops.feature_maps_format([x.cuda() for x in maps])
            res = runner.step(runner.img, metas, cameras=C.mask_rows(kept))
            outs = captured["outs"]
            assert runner.stats["overflow"] == 0
            assert ("camera_valid" in runner.inputs.metas(metas["img_metas"], runner.wh, runner.wh_host)) == runner.cam_masked == (f >= 1)
            for b in range(bs):
                groups = []
                for alloc in outs["alloc_list"]:
                    gs = alloc.group_start.cpu().numpy()
                    groups.append((int(gs[b * 6]), int(gs[(b + 1) * 6])))
                    sizes = np.diff(gs[b * 6:(b + 1) * 6 + 1])
                    assert all((sizes[c] == 0) == (c not in kept[b]) for c in range(6)), (f, b, sizes)
                _compare(outs, wants[b][f], ("stream", b, f), rows=b, groups=groups)
                ids, want_ids = outs["instance_id"][b].cpu().tolist(), wants[b][f]["instance_id"][0].tolist()
                for i, w in zip(ids, want_ids):
                    assert (i < 0) == (w < 0), (f, b)
                    if w >= 0:
                        assert relabel[b].setdefault(w, i) == i, (f, b, w, i)
                assert len(set(relabel[b].values())) == len(relabel[b])
                cams2d = res[b]["img_bbox"]["camidx_2d"].long().tolist()   # the 2D list of a masked camera is empty
                assert not set(cams2d) - set(kept[b]), (f, b)


def test_head_refusals():
    spec, head, _ = _setup()
    maps, metas = _frame(2, 0, spec["image_wh"])
    from simpb_amd.plugin import ops
    fm = ops.feature_maps_format([x.cuda() for x in maps])
    dm = metas_to(metas, "cuda")
    ok = torch.ones(2, 6, dtype=torch.uint8, device="cuda")
    for bad in (ok.cpu(), ok.bool(), ok[:, :5].contiguous(), ok[:1], torch.ones(6, 2, dtype=torch.uint8, device="cuda").t()):
        with pytest.raises(ValueError):
            head(fm, dict(dm, camera_valid=bad))
    layer = next(l for op, l in zip(head.operation_order, head.layers) if op == "deformable")
    with pytest.raises(NotImplementedError):   # the PyTorch composition of the layer (no image_wh) has no mask
        layer(torch.zeros(2, 4, 256, device="cuda"), torch.zeros(2, 4, 11, device="cuda"), torch.zeros(2, 4, 256, device="cuda"), fm,
              dict(projection_mat=dm["projection_mat"], camera_valid=ok))


# ------------------------------------------------------------------------------------------------------------ 2. runners
WH, SRC = (352, 128), (300, 800)
AUG = dict(resize=0.44, crop=(0, 4, 352, 132))
SPEC = dict(num_anchor=128, num_temp=64, num_output=32)
K4 = (0, 1, 2, 3)
SCHEDULE = [C.ALL, K5, K5, C.ALL, C.ALL, (0, 1, 2, 3, 4), K4, C.ALL, K5, K4, C.ALL, K5]


@functools.lru_cache(maxsize=None)
def _pristine():
    """The small detector (real ResNet50 + FPN, fp16 backbone; the head of SPEC), built once and never run: every runner gets
    its own deep copy."""
    from simpb_amd import configs, plugin
    cfg = configs.simpb_plus(anchor=synth.anchors(SPEC["num_anchor"]))
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


@functools.lru_cache(maxsize=None)
def _raw(f):
    return synth.raw_frames(1, f % 3, SRC)


def _metas(f):
    metas = synth.frame_metas(1, f, WH)
    for m in metas["img_metas"]:
        m["aug_config"] = dict(AUG)
    return metas


def _run(kind, use_graph, fill, cameras="schedule", frames=len(SCHEDULE)):
    """The schedule through one runner. fill: seed of the bytes a masked camera's slot holds (new ones every frame), or None:
    the slot keeps the camera's image. Returns the runner and per frame (rec3d, rec2d, result)."""
    from simpb_amd import runner as RN
    cls = dict(plain=RN.FrameRunner, pipe=RN.PipelinedRunner, split=RN.SplitPipelinedRunner)[kind]
    r = cls(copy.deepcopy(_pristine()), 1, (WH[1], WH[0]), capacity=256, device=torch.device("cuda"), use_graph=use_graph,
            raw_input=SRC)
    g = torch.Generator().manual_seed(fill) if fill is not None else None
    out, graphs = [], []
    for f in range(frames):
        kept = SCHEDULE[f]
        raw, metas = _raw(f).clone(), _metas(f)
        for c in range(6):
            if c not in kept and g is not None:
                raw[0, c] = torch.randint(0, 256, raw[0, c].shape, generator=g, dtype=torch.uint8)
                metas["projection_mat"][0, c] = NAN
        cams = dict(schedule=C.mask_rows([kept]), none=None, ones=[[True] * 6])[cameras]
        res = r.step(raw.cuda(), metas, cameras=cams)
        if res is not None:
            out.append((r.last_rec3d.clone(), r.last_rec2d.clone(), res[0]["img_bbox"]))
        graphs.append(r.graph if kind == "plain" else tuple(r.head_graph))
    if hasattr(r, "flush"):
        res = r.flush()
        out.append((r.last_rec3d.clone(), r.last_rec2d.clone(), res[0]["img_bbox"]))
    assert len(out) == frames and r.stats["overflow"] == 0, r.stats
    return r, out, graphs


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _assert_same_runs(a, b, what):
    for f, ((a3, a2, ra), (b3, b2, rb)) in enumerate(zip(a, b)):
        assert _same_bytes(a3, b3), (what, f, "rec3d")
        assert _same_bytes(a2, b2), (what, f, "rec2d")
        assert bool(torch.isfinite(a3[..., :13]).all()) and bool(torch.isfinite(a2).all()), (what, f)   # (columns 13-14: id bits)
        assert torch.equal(ra["instance_ids"], rb["instance_ids"]) and torch.equal(ra["camidx_2d"], rb["camidx_2d"]), (what, f)
        assert not set(ra["camidx_2d"].long().tolist()) - set(SCHEDULE[f]), (what, f)   # a masked camera's 2D list is empty


@pytest.mark.parametrize("kind", ["plain", "pipe", "split"])
def test_replayed_graphs_equal_eager_frames_whatever_the_masked_slots_hold(kind):
    """Eager frames with one filling of the masked slots against replayed graphs with another: the same bytes out. The graphs
    are dropped once (at the first masked frame, before any exists) and never captured again: from then on one captured
    graph per slot serves every mask of the schedule, the full rig (all ones) included."""
    re_, eager, _ = _run(kind, False, fill=1)
    rg, graph, graphs = _run(kind, True, fill=2)
    assert re_.stats["replay"] == 0 and rg.stats["replay"] >= 4, (re_.stats, rg.stats)
    assert rg.cam_masked and re_.cam_masked
    _assert_same_runs(eager, graph, kind)
    slots = list(zip(*graphs)) if kind != "plain" else [graphs]
    for seq in slots:   # once a slot's graph exists it is the same object to the end
        first = next(i for i, x in enumerate(seq) if x is not None)
        assert all(x is seq[first] for x in seq[first:]), kind
        replayed_masks = {SCHEDULE[f] for f in range(first, len(SCHEDULE))}
    assert len(replayed_masks) >= 2 and C.ALL in replayed_masks


def test_a_missing_camera_changes_the_result_and_a_full_mask_does_not():
    """cameras = all true is cameras = None bit for bit over the whole schedule (no graph is dropped, nothing is staged); the
    masked run differs from it in the masked frames."""
    r0, none, _ = _run("plain", True, fill=None, cameras="none")
    r1, ones, _ = _run("plain", True, fill=None, cameras="ones")
    assert not r0.cam_masked and not r1.cam_masked and r0.stats == r1.stats and r1.stats["replay"] >= 4
    for f, ((a3, a2, _), (b3, b2, _)) in enumerate(zip(none, ones)):
        assert _same_bytes(a3, b3) and _same_bytes(a2, b2), f
    _, masked, _ = _run("plain", True, fill=None, frames=3)
    assert _same_bytes(masked[0][0], none[0][0]) and not _same_bytes(masked[1][0], none[1][0])


def test_runner_refusals():
    from simpb_amd import runner as RN
    r = RN.SplitPipelinedRunner(copy.deepcopy(_pristine()), 1, (WH[1], WH[0]), capacity=256, device=torch.device("cuda"),
                                use_graph=True, raw_input=SRC)
    raw = _raw(0).cuda()
    with pytest.raises(ValueError):
        r.step(raw, _metas(0), cameras=[[True] * 5])
    with pytest.raises(ValueError):
        r.step(raw, _metas(0), cameras=[[True] * 6, [True] * 6])
    with pytest.raises(ValueError):   # a stream without any frame is paused, not masked
        r.step(raw, _metas(0), cameras=[[False] * 6])
    with pytest.raises(NotImplementedError):   # the single-stream runner still takes no paused stream
        r.step(raw, _metas(0), active=[False], cameras=[[True] * 6])
    assert not r.cam_masked and not r.queue
    assert r.step(raw, _metas(0), cameras=[[False] + [True] * 5]) is None and r.cam_masked   # a cold frame may have masked cameras
    assert r.flush()[0]["img_bbox"]["boxes_3d"].shape == (SPEC["num_output"], 10)
