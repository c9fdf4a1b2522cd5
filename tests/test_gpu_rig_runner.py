"""GPU: the frame runners on a rig of cameras that differ (raw_rig=[preprocess.CameraSource, ...]): R50 at 704 x 256 on the
synthetic generator's pictures. The witness is the runner fed fp32 images that tests/preprocess_ref.py makes camera by camera
from the BGR picture of every surface (tests/yuv_ref.py, surface_ref.p010_to_bgr): the backbone then sees identical f16
operands, so device records and detections are equal bit for bit over the cold frame, eager warm frames and replayed graphs.
A uniform rig is also compared with the raw_surfaces runner it generalises. Every surface handed to a runner stays referenced
until the test ends."""
import numpy as np
import pytest
import torch

from simpb_amd import preprocess as P
from simpb_amd import synth
from tests import preprocess_ref as R
from tests import surface_ref as S
from tests import yuv_ref as Y

pytestmark = pytest.mark.gpu

NORM = P.IMG_NORM_CFG
R50 = dict(resize=0.44, crop=(0, 140, 704, 396))
PADDED = dict(pitch=1792, luma_rows=912)
# (src_hw, format, colour, layout, aug_config) of a camera
NUS = ((900, 1600), "nv12", "jfif", None, R50)
NUS_PADDED = ((900, 1600), "nv12", "jfif", PADDED, R50)
HD10 = ((1080, 1920), "p010", "bt709", dict(pitch=4096, luma_rows=1088), dict(resize=0.44, crop=(70, 140, 774, 396)))
HD8 = ((1080, 1920), "nv12", "jfif", None, dict(resize=0.44, crop=(70, 140, 774, 396)))
HD720 = ((720, 1280), "bgr", "jfif", None, dict(resize=0.55, crop=(0, 140, 704, 396)))
MIXED = (NUS,) * 3 + (HD10,) * 3                 # one record rule: resize 0.44 and crop_y0 140 for every camera
TWO_RULES = (NUS,) * 3 + (HD10,) + (HD720,) * 2
_cache = {}


def source(spec):
    hw, fmt, colour, layout, aug = spec
    return P.CameraSource(hw, aug, fmt, colour, layout)


def picture(spec, f, c):
    """Camera c's picture of frame f % 3 as (its surface u8 [bytes] on the host, the fp32 image [3, 256, 704] the reference's
    pipeline makes of the BGR picture the surface holds)."""
    key = (spec[:3], repr(spec[3:]), f % 3, c)
    if key not in _cache:
        hw, fmt, colour, _, aug = spec
        if ("bgr", hw, f % 3) not in _cache:
            _cache["bgr", hw, f % 3] = synth.raw_frames(1, f % 3, src_hw=hw, num_cams=6)[0].numpy()
        bgr = _cache["bgr", hw, f % 3][c]
        layout = source(spec).surface
        if fmt == "bgr":
            surf = S.pack(bgr, layout, 0xEE)
        else:
            nv12 = Y.bgr_to_nv12(bgr, colour)
            if fmt == "p010":
                surf = S.pack(S.to_p010(nv12, np.random.RandomState(40 + c)), layout, 0xEE)
                bgr = S.p010_to_bgr(surf, layout, colour)
            else:
                surf = S.pack(nv12, layout, 0xEE)
                bgr = Y.yuv420sp_to_bgr(nv12, colour)
        _cache[key] = (torch.from_numpy(surf), torch.from_numpy(R.pipeline_nchw(bgr, aug, NORM)))
    return _cache[key]


def fp32_frame(specs, f, bs=1):
    """f32 [bs, 6, 3, 256, 704]: stream s shows frame f + s."""
    return torch.stack([torch.stack([picture(spec, f + s, c)[1] for c, spec in enumerate(specs)]) for s in range(bs)])


class Surfaces:
    """Every frame's surfaces as separate device tensors, odd cameras one byte (p010: two) off their allocation's alignment;
    all of them stay referenced here until the test ends."""

    def __init__(self, specs):
        self.specs, self.handed = specs, []

    def frame(self, f, bs=1):
        rows = []
        for s in range(bs):
            row = []
            for c, spec in enumerate(self.specs):
                surf = picture(spec, f + s, c)[0]
                off = (c % 2) * (2 if spec[1] == "p010" else 1)
                buf = torch.empty(surf.numel() + off, dtype=torch.uint8, device="cuda")
                buf[off:].copy_(surf)
                row.append(buf[off:])
            rows.append(row)
        self.handed.append(rows)
        return [list(r) for r in rows]


def _model():
    from simpb_amd import configs, plugin
    cfg = configs.simpb_plus(anchor=synth.anchors(900))
    model = plugin.build_detector(cfg["model"]).eval()
    synth.load_procedural(model)
    model.cuda()
    model.fuse_conv_bn()
    model.half_backbone()
    return model


def _runner(name, bs=1, **kw):
    from simpb_amd import runner
    return getattr(runner, name)(_model(), bs, (256, 704), capacity=1536, device=torch.device("cuda"), use_graph=True,
                                 independent_streams=bs > 1, **kw)


def _drive(r, feed, frames, bs=1, metas=None, **step_kw):
    """`frames` steps of runner r; feed(f) gives the step's img. Returns per frame (results, rec3d, rec2d)."""
    got = []
    keep = lambda res: got.append((res, r.last_rec3d.clone(), r.last_rec2d.clone()))   # noqa: E731
    for f in range(frames):
        kw = {k: v[f] for k, v in step_kw.items()}
        res = r.step(feed(f), metas(f) if metas is not None else synth.frame_metas(bs, f), **kw)
        if res is not None:
            keep(res)
    if hasattr(r, "flush"):
        keep(r.flush())
    assert len(got) == frames
    return got


def _compare(a, b, name, streams=None, rec2d=True):
    for f, ((ra, a3, a2), (rb, b3, b2)) in enumerate(zip(a, b)):
        rows = range(a3.shape[0]) if streams is None else [i for i in range(a3.shape[0]) if streams[f][i]]
        for i in rows:
            assert torch.equal(a3[i], b3[i]), (name, f, i, "rec3d")
            assert not rec2d or torch.equal(a2[i], b2[i]), (name, f, i, "rec2d")
        for i, (sa, sb) in enumerate(zip(ra, rb)):
            assert (sa is None) == (sb is None), (name, f, i)
            if sa is None:
                continue
            xa, xb = sa["img_bbox"], sb["img_bbox"]
            assert xa.keys() == xb.keys(), (name, f)
            for k in xa:
                if not rec2d and k == "boxes_2d":
                    continue
                x, y = xa[k], xb[k]
                if torch.is_tensor(x) or isinstance(x, np.ndarray):
                    x, y = torch.as_tensor(x), torch.as_tensor(y)
                    assert x.shape == y.shape and torch.equal(x, y), (name, f, i, k)
                else:
                    assert np.array_equal(np.asarray(x), np.asarray(y)), (name, f, i, k)


# FrameRunner replays from its third frame on, a pipelined runner from the fifth (one graph per feature slot): the fewest
# frames with three replays
@pytest.mark.parametrize("name,frames", [("FrameRunner", 5), ("PipelinedRunner", 7), ("SplitPipelinedRunner", 7)])
def test_uniform_rig_equals_the_raw_surfaces_runner(name, frames):
    specs = (NUS_PADDED,) * 6
    base = _runner(name, raw_input=(900, 1600), raw_format="nv12", raw_layout=PADDED, raw_surfaces=True)
    one = Surfaces(specs)
    a = _drive(base, lambda f: one.frame(f), frames)
    assert base.stats["replay"] >= 3, base.stats
    rig = _runner(name, raw_rig=[source(s) for s in specs])
    assert rig.img is None and rig.raw.dtype == torch.int64 and tuple(rig.raw.shape) == (1, 6) and rig.raw_input is None
    two = Surfaces(specs)
    b = _drive(rig, lambda f: two.frame(f), frames)
    assert rig.stats == base.stats and rig.stats["replay"] >= 3, (rig.stats, base.stats)
    _compare(a, b, name + " uniform rig")
    # refused before anything is enqueued: a tensor in place of the list, a host surface, a short one, a missing one, five
    before = dict(rig.stats)
    row = two.frame(frames)[0]
    metas = synth.frame_metas(1, frames)
    small = torch.zeros(source(NUS_PADDED).surface.sample_end - 1, dtype=torch.uint8, device="cuda")
    for bad, err in ((torch.zeros(1, 6, 8, dtype=torch.uint8, device="cuda"), ValueError), ([[t.cpu() for t in row]], RuntimeError),
                     ([row[:5] + [small]], ValueError), ([row[:5] + [None]], ValueError), ([row[:5]], ValueError)):
        with pytest.raises(err):
            rig.step(bad, metas)
    assert rig.stats == before and len(getattr(rig, "queue", [])) == 0


@pytest.mark.parametrize("name,frames", [("FrameRunner", 4), ("SplitPipelinedRunner", 6)])
def test_mixed_sizes_one_record_rule(name, frames):
    """Three 1600 x 900 NV12 cameras beside three 1920 x 1080 P010 (bt709) cameras on a padded layout, all with resize 0.44 and
    crop_y0 140: the criterion of test_runner_raw_input_equals_fp32_input."""
    ref = _runner(name)
    a = _drive(ref, lambda f: fp32_frame(MIXED, f).cuda(), frames)
    rig = _runner(name, raw_rig=[source(s) for s in MIXED])
    surf = Surfaces(MIXED)
    b = _drive(rig, lambda f: surf.frame(f), frames)
    assert rig.stats == ref.stats and rig.stats["replay"] >= 1, (rig.stats, ref.stats)
    assert rig.plan.key[0] == "rig" and len(set(rig.plan.src_rows)) == 2
    _compare(a, b, name + " mixed rig")


def test_mixed_record_rules():
    """Cameras 4 and 5 are 1280 x 720 BGR at resize 0.55: the 3D half equals the fp32 runner's; the 2D rows of each camera equal
    the rows of the fp32 run whose metas carry that camera's (resize, crop)."""
    frames = 4
    rig = _runner("FrameRunner", raw_rig=[source(s) for s in TWO_RULES])
    surf = Surfaces(TWO_RULES)
    got = _drive(rig, lambda f: surf.frame(f), frames)
    assert rig.stats["replay"] >= 2
    runs = {}
    for rule, aug in (("0.44", R50), ("0.55", HD720[4])):
        def metas(f, aug=aug):
            m = synth.frame_metas(1, f)
            m["img_metas"][0]["aug_config"] = dict(aug)
            return m
        ref = _runner("FrameRunner")
        runs[rule] = _drive(ref, lambda f: fp32_frame(TWO_RULES, f).cuda(), frames, metas=metas)
        assert ref.stats == rig.stats
        _compare(runs[rule], got, "3D half, rule " + rule, rec2d=False)
    differ = 0
    for f in range(frames):
        g2, a2, b2 = got[f][2][0], runs["0.44"][f][2][0], runs["0.55"][f][2][0]
        cam = g2[:, 7]
        assert torch.equal(cam, a2[:, 7]) and torch.equal(cam, b2[:, 7])
        low, high = cam < 4, cam >= 4
        assert torch.equal(g2[low], a2[low]) and torch.equal(g2[high], b2[high]), f
        differ += int((a2[high, :4] != b2[high, :4]).any())
        # the detections' 2D boxes, per camera as well
        box, boxa, boxb = (r[f][0][0]["img_bbox"]["boxes_2d"] for r in (got, runs["0.44"], runs["0.55"]))
        high = got[f][0][0]["img_bbox"]["camidx_2d"] >= 4
        assert torch.equal(box[~high], boxa[~high]) and torch.equal(box[high], boxb[high]), f
    assert differ, "the two rules never gave different boxes: the comparison shows nothing"


def test_two_streams_pause_and_a_missing_camera():
    """Stream 1 pauses for frames 3 and 4 (its row is None), stream 0 loses camera 4 (a 1920 x 1080 P010 camera) in frames 2 and
    3: None in the rig's table is an image the ingest skips. Equal to the fp32-input runner under the same schedule."""
    frames = 6
    active = [None, None, None, (True, False), (True, False), None]
    lost = [[True, True, True, True, False, True], [True] * 6]
    cameras = [None, None, lost, lost, None, None]
    ref = _runner("PipelinedRunner", bs=2)
    a = _drive(ref, lambda f: fp32_frame(MIXED, f, 2).cuda(), frames, bs=2, active=active, cameras=cameras)
    rig = _runner("PipelinedRunner", bs=2, raw_rig=[source(s) for s in MIXED])
    surf = Surfaces(MIXED)

    def feed(f):
        rows = surf.frame(f, 2)
        if cameras[f] is not None:
            rows[0][4] = None
        if active[f] is not None:
            rows[1] = None if f == 3 else [None] * 6
        return rows

    b = _drive(rig, feed, frames, bs=2, active=active, cameras=cameras)
    assert rig.stats == ref.stats, (rig.stats, ref.stats)
    _compare(a, b, "paused + masked", streams=[(True, True) if m is None else m for m in active])
    assert [r is None for r in b[3][0]] == [False, True]
    with pytest.raises(ValueError, match="neither paused nor masked"):
        rows = surf.frame(frames, 2)
        rows[1][0] = None
        rig.step(rows, synth.frame_metas(2, frames))


def test_set_raw_rig_between_frames():
    """Camera 2 is replaced by a 1920 x 1080 camera (NV12, the same record rule) before the last frame of a warm, replaying
    stream: the graphs are dropped and captured again, and every frame equals the fp32-input runner fed the reference's
    images of the very pictures the rig runner was shown -- the same bank state, frame for frame."""
    frames, switch = 4, 3
    before, after = (NUS,) * 6, (NUS,) * 2 + (HD8,) + (NUS,) * 3
    specs = lambda f: before if f < switch else after   # noqa: E731
    ref = _runner("FrameRunner")
    a = _drive(ref, lambda f: fp32_frame(specs(f), f).cuda(), frames)
    r = _runner("FrameRunner", raw_rig=[source(s) for s in before])
    surf = {False: Surfaces(before), True: Surfaces(after)}
    got = []
    for f in range(frames):
        if f == switch:
            assert r.graph is not None and r.stats["replay"] >= 1
            old = r.plan
            r.set_raw_rig([source(s) for s in before])          # an equal key: nothing happens
            assert r.graph is not None and r.plan is old
            r.set_raw_rig([source(s) for s in after])
            assert r.graph is None and r.plan is not old and r.plan.src_rows[2] != old.src_rows[2]
            with pytest.raises(ValueError, match="camera 2 of the rig"):
                r.step(surf[False].frame(f), synth.frame_metas(1, f))        # the old camera's surface is no longer taken
            with pytest.raises(ValueError, match="6"):
                r.set_raw_rig([source(s) for s in after[:5]])
        res = r.step(surf[f >= switch].frame(f), synth.frame_metas(1, f))
        got.append((res, r.last_rec3d.clone(), r.last_rec2d.clone()))
    assert r.stats == ref.stats and r.stats["replay"] >= 2, (r.stats, ref.stats)
    _compare(a, got, "rig change")


def test_set_raw_rig_equals_a_runner_built_with_the_new_rig():
    """The same change against a runner that had the new rig from the start and was fed the same state: camera 2 delivers
    nothing (None, masked through cameras=) until the frame at which it comes back as the 1920 x 1080 camera, so both runners
    hold the same bank when that frame arrives."""
    frames, switch = 4, 3
    before, after = (NUS,) * 6, (NUS,) * 2 + (HD8,) + (NUS,) * 3
    lost = [[True, True, False, True, True, True]]
    cameras = [lost] * switch + [None] * (frames - switch)
    surf = Surfaces(after)

    def feed(f):
        rows = surf.frame(f)
        if f < switch:
            rows[0][2] = None
        return rows

    new = _runner("FrameRunner", raw_rig=[source(s) for s in after])
    a = _drive(new, feed, frames, cameras=cameras)
    r = _runner("FrameRunner", raw_rig=[source(s) for s in before])
    got = []
    for f in range(frames):
        if f == switch:
            assert r.graph is not None
            r.set_raw_rig([source(s) for s in after])
            assert r.graph is None and r.plan.key == new.plan.key
        res = r.step(feed(f), synth.frame_metas(1, f), cameras=cameras[f])
        got.append((res, r.last_rec3d.clone(), r.last_rec2d.clone()))
    assert r.stats == new.stats and r.stats["replay"] >= 2, (r.stats, new.stats)
    _compare(a, got, "rig change against the new rig from the start")


def test_set_raw_rig_is_refused_with_a_frame_in_flight():
    specs = (NUS,) * 6
    r = _runner("PipelinedRunner", raw_rig=[source(s) for s in specs])
    surf = Surfaces(specs)
    assert r.step(surf.frame(0), synth.frame_metas(1, 0)) is None and len(r.queue) == 1
    new = [source(s) for s in (NUS,) * 5 + (HD8,)]
    old = r.plan
    with pytest.raises(RuntimeError, match="flush"):
        r.set_raw_rig(new)
    assert r.plan is old and len(r.queue) == 1
    assert r.flush() is not None and not r.queue
    r.set_raw_rig(new)
    assert r.plan is not old and r.plan.key == P.RigPlan(new).key
    with pytest.raises(ValueError, match="raw_input"):
        r.set_raw_layout(PADDED)


def test_constructor_refusals():
    from simpb_amd import runner
    model = _model()
    rig = [source(NUS)] * 6
    dev = torch.device("cuda")
    for cls in (runner.FrameRunner, runner.PipelinedRunner, runner.SplitPipelinedRunner):
        for kw in (dict(raw_input=(900, 1600)), dict(raw_format="nv12"), dict(raw_colour="bt709"), dict(raw_layout=PADDED),
                   dict(raw_surfaces=True)):
            with pytest.raises(ValueError, match="raw_rig"):
                cls(model, 1, (256, 704), device=dev, raw_rig=rig, **kw)
        with pytest.raises(ValueError, match="5 cameras, the model 6"):
            cls(model, 1, (256, 704), device=dev, raw_rig=rig[:5])
        with pytest.raises(ValueError, match=r"\(256, 704\).*\(256, 640\)"):
            cls(model, 1, (256, 640), device=dev, raw_rig=rig)
    with pytest.raises(ValueError, match="one output size"):
        runner.FrameRunner(model, 1, (256, 704), device=dev, raw_rig=rig[:5] + [source(((900, 1600), "nv12", "jfif", None, dict(resize=0.44)))])
    with pytest.raises(NotImplementedError, match="device kernels"):
        model.head.decoder.decode_box2d(torch.zeros(1, 4), P.RigPlan(rig))
    with pytest.raises(ValueError, match="raw_rig runner"):
        runner.FrameRunner(model, 1, (256, 704), device=dev).set_raw_rig(rig)
