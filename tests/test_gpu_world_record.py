"""GPU: the world record (csrc/world.hip) against its host statement (results.world_record_host) on the same inputs, and through
the three runners -- captured graphs, poses that change every step, a paused stream -- against format_sample."""
import functools

import numpy as np
import pytest
import torch

from simpb_amd import results, synth
from tests import world_cases as W
from tests.helpers import build_product_head

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------- 1. kernel against the host
def _device_record(rec, pose, tables, threshold, active=None):
    from simpb_amd.plugin.detection3d import SparseBox3DDecoder
    world, count = SparseBox3DDecoder(num_output=rec.shape[1]).world_record(
        torch.from_numpy(rec).cuda(), torch.from_numpy(pose).cuda(),
        torch.tensor(active, dtype=torch.uint8).cuda() if active is not None else None, tables, threshold)
    torch.cuda.synchronize()
    return world.cpu().numpy(), count.cpu().numpy()


def _patterns(k):
    """Which rows a case keeps: all, none, every other, and only the last row of each wave with the first of the next."""
    r = np.arange(k)
    return dict(all=np.ones(k, bool), none=np.zeros(k, bool), alternate=r % 2 == 0,
                wave_edges=((r % 64 == 63) | (r % 64 == 0)) & (r > 0))


@pytest.mark.parametrize("k", [1, 63, 64, 65, 300, 512])
@pytest.mark.parametrize("streams", [1, 3])
def test_kernel_equals_host_over_keep_patterns(streams, k):
    rng = np.random.default_rng(1000 * streams + k)
    infos = [W.random_pose(rng) for _ in range(streams)]
    pose = np.stack([results.pose_row(i) for i in infos])
    # boxes within 20 m (inside every class range), detection mode (no class dropped): the score lane alone decides
    base = np.stack([W.random_record(rng, k, i, spread=20.0) for i in infos])
    tables = results.world_tables(W.CLASSES, False)
    for name, keep in _patterns(k).items():
        rec = base.copy()
        rec[:, :, 12] = np.where(keep, 0.9, 0.1)
        active = None if streams == 1 else [1, 0, 1]
        want = results.world_record_host(rec, pose, tables, W.THRESHOLD, active)
        if active is None:
            assert want[1].tolist() == [int(keep.sum())], name
        else:
            assert want[1].tolist() == [int(keep.sum()), -1, int(keep.sum())], name
        W.assert_records_equal(*_device_record(rec, pose, tables, W.THRESHOLD, active), *want)


@pytest.mark.parametrize("tracking,threshold", [(False, None), (True, W.THRESHOLD)])
def test_kernel_equals_host_and_format_sample_on_mixed_boxes(tracking, threshold):
    """All three cuts at work at once (boxes out to 60 m, every class, both sides of the speed cut), K = 300, 3 streams."""
    rng = np.random.default_rng(77)
    infos = [dict(W.random_pose(rng), token=f"t{s}") for s in range(3)]
    pose = np.stack([results.pose_row(i) for i in infos])
    rec = np.stack([W.random_record(rng, 300, i) for i in infos])
    tables = results.world_tables(W.CLASSES, tracking)
    want = results.world_record_host(rec, pose, tables, threshold)
    world, count = _device_record(rec, pose, tables, threshold)
    W.assert_records_equal(world, count, *want)
    for s, info in enumerate(infos):
        assert 0 < count[s] < 300
        W.assert_same_annos(results.annos_from_world(world[s], count[s], info["token"], W.CLASSES, tracking),
                            results.format_sample(W.det_of(rec[s]), info, W.CLASSES, tracking, threshold), tracking)


def test_kernel_on_boxes_exactly_on_a_cut():
    rec, kept = W.exact_cuts()
    pose = results.pose_row(W.IDENTITY_POSE)[None]
    tables = results.world_tables(W.CLASSES, False)
    world, count = _device_record(rec[None], pose, tables, 0.25)
    assert count.tolist() == [len(kept)]
    W.assert_records_equal(world, count, *results.world_record_host(rec[None], pose, tables, 0.25))
    assert np.array_equal(world[0, :2, 0:3], rec[kept, 0:3].astype(np.float64))


# --------------------------------------------------------------------------------------------------------- 2. runners
WH, BS, CAP = (352, 128), 2, 256
SPEC = dict(num_anchor=128, num_temp=64, num_output=32)
STEPS = 6
WORLD = dict(classes=W.CLASSES, tracking=True, threshold=0.05)


@functools.lru_cache(maxsize=None)
def _maps(step):
    return tuple(m.half().float() for m in synth.feature_maps_nchw(BS, step, WH))


@functools.lru_cache(maxsize=None)
def _tokens(step):
    from simpb_amd.plugin import ops
    return ops.feature_maps_format([x.cuda() for x in _maps(step)])[0].clone()


class _Staged(torch.nn.Module):
    """Detector stand-in of tests/test_gpu_stream_activity.py: tokens served from fixed-address buffers per image slot."""

    def __init__(self, head):
        super().__init__()
        self.head, self.bufs, self.staged = head, {}, torch.empty_like(_tokens(0))

    def stage(self, tokens):
        self.staged.copy_(tokens)

    def extract_feat(self, img):
        from simpb_amd.plugin import ops
        key = img.data_ptr()
        if key not in self.bufs:
            fm = ops.feature_maps_format([torch.zeros_like(x).cuda() for x in _maps(0)])
            fm[0].simpb_f16 = torch.zeros_like(fm[0], dtype=torch.float16)
            self.bufs[key] = fm
        fm = self.bufs[key]
        fm[0].copy_(self.staged, non_blocking=True)
        fm[0].simpb_f16.copy_(self.staged, non_blocking=True)
        return fm


def _runner(kind, world_output, **kw):
    from simpb_amd.runner import FrameRunner, PipelinedRunner, SplitPipelinedRunner
    cls = dict(plain=FrameRunner, pipe=PipelinedRunner, split=SplitPipelinedRunner)[kind]
    model = _Staged(build_product_head(SPEC))
    return model, cls(model, BS, (WH[1], WH[0]), capacity=CAP, device=torch.device("cuda"), use_graph=True,
                      independent_streams=True, **({} if world_output == "absent" else dict(world_output=world_output)), **kw)


@functools.lru_cache(maxsize=None)
def _metas(step):
    """The frame's metas with a pose per stream that is another one at every step."""
    metas = synth.frame_metas(BS, step, WH)
    rng = np.random.default_rng(300 + step)
    for s, m in enumerate(metas["img_metas"]):
        m.update(W.random_pose(rng), token=f"s{s}-f{step}")
    return metas


def _drive(kind, world_output, schedule=None):
    """STEPS frames through a runner; per frame the returned list (the pipelined runners' one-frame delay undone)."""
    model, r = _runner(kind, world_output)
    outs = []
    for step in range(STEPS):
        model.stage(_tokens(step))
        torch.cuda.synchronize()   # (the stand-in's staging buffer is shared by the frames in flight)
        kw = dict(active=schedule[step]) if schedule is not None else {}
        outs.append(r.step(r.img, _metas(step), **kw))
    if kind != "plain":
        outs = outs[1:] + [r.flush()]
    return r, outs


def _check_frame(res, step, mask=(True,) * BS):
    for s, on in enumerate(mask):
        if not on:
            assert res[s] is None
            continue
        det, info = res[s]["img_bbox"], _metas(step)["img_metas"][s]
        w = det["world"]
        assert w["record"].shape == (w["count"], 16) and w["record"].dtype == np.float64
        want = results.format_sample(det, info, W.CLASSES, WORLD["tracking"], WORLD["threshold"])
        W.assert_same_annos(results.annos_from_world(w["record"], w["count"], info["token"], W.CLASSES, WORLD["tracking"]),
                            want, WORLD["tracking"])


@pytest.mark.parametrize("kind", ["plain", "pipe", "split"])
def test_runner_world_record_equals_format_sample_on_every_step(kind):
    r, outs = _drive(kind, WORLD)
    assert r.stats["replay"] >= 2 and r.stats["overflow"] == 0, r.stats   # replayed steps are among those checked
    kept = 0
    for step, res in enumerate(outs):
        _check_frame(res, step)
        kept += sum(x["img_bbox"]["world"]["count"] for x in res)
    assert 0 < kept < STEPS * BS * SPEC["num_output"]   # the cuts cut, and not everything
    torch.cuda.synchronize()
    assert r.last_world.shape == (BS, SPEC["num_output"], 16) and r.last_world_count.tolist() == \
        [x["img_bbox"]["world"]["count"] for x in outs[-1]]


@pytest.mark.parametrize("kind", ["plain", "pipe"])
def test_runner_paused_stream_has_no_record(kind):
    schedule = [(True, True)] * 4 + [(True, False)] + [(True, True)]
    r, outs = _drive(kind, WORLD, schedule)
    for step, res in enumerate(outs):
        _check_frame(res, step, schedule[step])
    r2, outs2 = _drive(kind, WORLD, schedule[:5] + [(True, False)])
    torch.cuda.synchronize()
    assert outs2[-1][1] is None and int(r2.last_world_count[1]) == -1 and int(r2.last_world_count[0]) >= 0


def test_missing_pose_is_refused_before_anything_is_enqueued():
    model, r = _runner("plain", WORLD)
    model.stage(_tokens(0))
    metas = synth.frame_metas(BS, 0, WH)   # no pose keys
    with pytest.raises(ValueError):
        r.step(r.img, metas)
    assert r.stats == dict(eager=0, replay=0, overflow=0) and r.prev_metas is None


def _same_bytes(a, b):
    a, b = torch.as_tensor(np.asarray(a)), torch.as_tensor(np.asarray(b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("kind", ["plain", "pipe", "split"])
def test_option_off_changes_nothing(kind):
    """world_output=None against a runner built without the keyword (the constructor call from before it existed) and against
    the option switched on: stats equal, every img_bbox entry bit for bit the same, no `world` key, no buffer."""
    r_old, old = _drive(kind, "absent")
    r_off, off = _drive(kind, None)
    r_on, on = _drive(kind, WORLD)
    assert r_old.stats == r_off.stats == r_on.stats
    assert not any("pose" in s.dev or "pose" in s.host for s in r_off.slot_inputs) and not hasattr(r_off, "last_world")
    for step in range(STEPS):
        for s in range(BS):
            a, b, c = old[step][s]["img_bbox"], off[step][s]["img_bbox"], on[step][s]["img_bbox"]
            assert "world" not in a and "world" not in b and "world" in c
            assert sorted(a) == sorted(b) == sorted(k for k in c if k != "world")
            for k in a:
                if k == "query_groups":
                    assert a[k] == b[k] == c[k], (step, s, k)
                else:
                    assert _same_bytes(a[k], b[k]) and _same_bytes(a[k], c[k]), (step, s, k)
    assert _same_bytes(r_old.last_rec3d.cpu(), r_off.last_rec3d.cpu()) and _same_bytes(r_old.last_rec2d.cpu(), r_off.last_rec2d.cpu())
