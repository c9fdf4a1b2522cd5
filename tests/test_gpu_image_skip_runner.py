"""GPU: the three runners with idle_images="skip" against the same runner with idle_images="compute", on the real backbone
(ResNet50 + FPN, fp16, BN folded) at 128 x 352, the smallest image the backbone's shape rules take. Two runners of the same
weights run one schedule of pauses and missing cameras, graphs on; everything an active stream gets back -- device records,
results, bank rows -- must be the same bytes, and the "skip" runner must stage nothing before the first dead image."""
import copy
import functools

import numpy as np
import pytest
import torch

from simpb_amd import synth

pytestmark = pytest.mark.gpu

WH, SRC = (352, 128), (300, 800)
AUG = dict(resize=0.44, crop=(0, 4, 352, 132))
SPEC = dict(num_anchor=128, num_temp=64, num_output=32)
CAMS = 6
ALL = (True,) * CAMS
STATE = ("cached_feature", "cached_anchor", "confidence", "instance_id")


def _down(*cams):
    return tuple(c not in cams for c in range(CAMS))


# (active, cameras) per frame: all live, stream 1 paused, stream 1 back with one camera down, both with a camera down,
# stream 0 paused, all live
SCHEDULE2 = [((True, True), None),
             ((True, False), None),
             ((True, True), (ALL, _down(2))),
             ((True, True), (_down(5), _down(0))),
             ((False, True), None),
             ((True, True), None)]
# the single-stream runner: cameras only
SCHEDULE1 = [((True,), None), ((True,), (_down(1),)), ((True,), (_down(1),)), ((True,), (_down(0, 4),)), ((True,), None),
             ((True,), (_down(3),))]


@functools.lru_cache(maxsize=None)
def _pristine():
    """The detector with the real backbone and a small head, built as tests/test_gpu_plane_runner.py builds its model, once
    and never run: every runner gets its own deep copy of the same weights."""
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
def _frames(bs, f, raw):
    return synth.raw_frames(bs, f % 3, SRC) if raw else synth.images(bs, f % 3, WH)


def _metas(bs, f):
    metas = synth.frame_metas(bs, f, WH)
    for m in metas["img_metas"]:
        m["aug_config"] = dict(AUG)
    return metas


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _bank(r):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in r.head.instance_bank._static.items()}


def _run(kind, idle, bs, schedule, raw, poison=False):
    """The schedule through one runner -> per frame dict(res, rec3d, rec2d[, bank]) and the bank behind the last frame.
    poison: the input slot of every dead image holds NaN (f32 images) or 0xFF bytes (raw frames)."""
    from simpb_amd import runner as RN
    cls = dict(plain=RN.FrameRunner, pipe=RN.PipelinedRunner, split=RN.SplitPipelinedRunner)[kind]
    kw = dict(raw_input=SRC) if raw else {}
    r = cls(copy.deepcopy(_pristine()), bs, (WH[1], WH[0]), capacity=256, device=torch.device("cuda"), use_graph=True,
            independent_streams=bs > 1, idle_images=idle, **kw)
    assert r.idle_images == idle
    out = []

    def keep(res):
        out.append(dict(res=res, rec3d=r.last_rec3d.clone(), rec2d=r.last_rec2d.clone(), bank=_bank(r) if kind == "plain" else None))

    dead_seen = False
    for f, (active, cameras) in enumerate(schedule):
        img = _frames(bs, f, raw).clone()
        dead = [(s, c) for s in range(bs) for c in range(CAMS) if not active[s] or (cameras is not None and not cameras[s][c])]
        if poison:
            for s, c in dead:
                img[s, c] = 255 if raw else float("nan")
        if not dead_seen and idle == "skip":
            # nothing of the feature exists before the first dead image: no table, no dropped graph, the ordinary counters
            assert not r.skipping and r.live_dev is None and r.live_pin is None and "image_skip" not in r.stats, (f, r.stats)
        dead_seen = dead_seen or bool(dead)
        res = r.step(img.cuda(), _metas(bs, f), active=None if all(active) else list(active),
                     cameras=None if cameras is None else [list(row) for row in cameras])
        if res is not None:
            keep(res)
    if hasattr(r, "flush"):
        keep(r.flush())
    assert len(out) == len(schedule) and r.stats["overflow"] == 0, r.stats
    return r, out, _bank(r)


def _equal_results(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x) or isinstance(x, np.ndarray):
            x, y = torch.as_tensor(x), torch.as_tensor(y)
            assert x.shape == y.shape and _same_bytes(x, y), (what, k)
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y)), (what, k)


def _assert_same(a, b, schedule, what):
    """Every active stream's records, results and (where taken) bank rows: the same bytes in both runs; a paused stream is
    None in both; a masked camera's 2D list is empty in both."""
    for f, ((active, cameras), x, y) in enumerate(zip(schedule, a, b)):
        for s, on in enumerate(active):
            if not on:
                assert x["res"][s] is None and y["res"][s] is None, (what, f, s)
                continue
            assert _same_bytes(x["rec3d"][s], y["rec3d"][s]), (what, f, s, "rec3d")
            assert _same_bytes(x["rec2d"][s], y["rec2d"][s]), (what, f, s, "rec2d")
            assert bool(torch.isfinite(x["rec3d"][s][..., :13]).all()) and bool(torch.isfinite(x["rec2d"][s]).all()), (what, f, s)
            _equal_results(x["res"][s]["img_bbox"], y["res"][s]["img_bbox"], (what, f, s))
            if cameras is not None:
                gone = {c for c in range(CAMS) if not cameras[s][c]}
                assert not gone & set(y["res"][s]["img_bbox"]["camidx_2d"].long().tolist()), (what, f, s)
            if x["bank"] is not None:
                for k in STATE:
                    assert _same_bytes(x["bank"][k][s], y["bank"][k][s]), (what, f, s, k)


def _assert_same_bank(a, b, what):
    for k in STATE:   # behind the last frame, in which every stream took part
        assert _same_bytes(a[k], b[k]), (what, k)
    assert int(a["prev_id"]) == int(b["prev_id"]), what


def _check_skip_runner(r, schedule, slots):
    first = next(f for f, (active, cameras) in enumerate(schedule) if not all(active) or cameras is not None)
    assert r.skipping and r.stats["image_skip"] == len(schedule) - first, r.stats   # every frame from the first dead image on
    assert len(r.live_dev) == len(r.live_pin) == slots
    for t, p in zip(r.live_dev, r.live_pin):
        assert t.dtype == torch.int32 and tuple(t.shape) == (1 + r.bs * CAMS,) and t.is_cuda and p.is_pinned()


@pytest.mark.parametrize("kind", ["plain", "pipe"])
def test_skip_equals_compute_over_pauses_and_missing_cameras(kind):
    """bs 2, independent streams, f32 images, graphs on. The dead images' input slots hold what the live frame would: the
    two runners see the same inputs and differ in the backbone's walk alone."""
    rc, compute, bank_c = _run(kind, "compute", 2, SCHEDULE2, raw=False)
    rs, skip, bank_s = _run(kind, "skip", 2, SCHEDULE2, raw=False)
    assert not rc.skipping and rc.live_dev is None and "image_skip" not in rc.stats
    _check_skip_runner(rs, SCHEDULE2, 1 if kind == "plain" else 2)
    assert rs.stats["replay"] >= (3 if kind == "plain" else 0), rs.stats
    if kind == "pipe":   # the backbone graphs were captured again behind the switch and read the tables
        assert all(g is not None for g in rs.bb_graph)
    _assert_same(compute, skip, SCHEDULE2, kind)
    _assert_same_bank(bank_c, bank_s, kind)


def test_split_runner_skip_equals_compute_over_missing_cameras():
    """SplitPipelinedRunner, bs 1, raw u8 frames, a camera-only schedule."""
    rc, compute, bank_c = _run("split", "compute", 1, SCHEDULE1, raw=True)
    rs, skip, bank_s = _run("split", "skip", 1, SCHEDULE1, raw=True)
    _check_skip_runner(rs, SCHEDULE1, 2)
    assert all(g is not None for g in rs.bb_graph)
    _assert_same(compute, skip, SCHEDULE1, "split")
    _assert_same_bank(bank_c, bank_s, "split")


@pytest.mark.parametrize("raw", [False, True], ids=["f32-nan", "u8-ff"])
def test_skip_reads_nothing_of_a_dead_image(raw):
    """The dead images' INPUT slots hold NaN (f32 images) or 0xFF bytes (raw frames) in the "skip" runner only; the "compute"
    runner gets the clean frames. The active streams' outputs are the same bytes and finite."""
    _, compute, bank_c = _run("plain", "compute", 2, SCHEDULE2, raw=raw)
    _, skip, bank_s = _run("plain", "skip", 2, SCHEDULE2, raw=raw, poison=True)
    _assert_same(compute, skip, SCHEDULE2, ("poison", raw))
    _assert_same_bank(bank_c, bank_s, ("poison", raw))


def test_an_all_live_run_never_switches():
    """idle_images="skip" with no dead image in the whole run: nothing is staged, no graph is dropped, and the counters are
    those of the "compute" runner."""
    schedule = [((True, True), None)] * 4
    rc, compute, _ = _run("plain", "compute", 2, schedule, raw=False)
    rs, skip, _ = _run("plain", "skip", 2, schedule, raw=False)
    assert not rs.skipping and rs.live_dev is None and rs.stats == rc.stats and rs.stats["replay"] >= 2, (rs.stats, rc.stats)
    _assert_same(compute, skip, schedule, "all live")
