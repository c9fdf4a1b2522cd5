"""GPU: the camera frame ingest (csrc/preprocess.hip) against the numpy restatement of the reference's host pipeline
(tests/preprocess_ref.py, itself pinned to Pillow and to the reference's own function by tests/test_preprocess_host.py), and
the runners' raw_input mode against the same runners fed the fp32 tensor that restatement makes. The path is integer
arithmetic plus a table, so every comparison is bit for bit; every test does a fixed, small amount of work."""
import ctypes

import numpy as np
import pytest
import torch

from simpb_amd import preprocess as P
from simpb_amd import synth
from tests import preprocess_ref as R
from tests.test_preprocess_host import golden_cases

pytestmark = pytest.mark.gpu

R50 = dict(resize=0.44, crop=(0, 140, 704, 396))
R101 = dict(resize=0.88, crop=(0, 280, 1408, 792))
NORM = P.IMG_NORM_CFG
_cache = {}


def frames6():
    """u8 [6, 900, 1600, 3]: three cameras of the synthetic generator, three of plain uniform noise."""
    if "frames" not in _cache:
        a = synth.raw_frames(1, 0)[0, :3].numpy()
        b = np.random.RandomState(11).randint(0, 256, (3, 900, 1600, 3)).astype(np.uint8)
        _cache["frames"] = np.ascontiguousarray(np.concatenate([a, b]))
    return _cache["frames"]


def expected(frames, aug, norm, key=None):
    """f16 [N, h, w, 4] the ingest must produce. The resize of `key`-ed frame sets is cached per (resize, crop): flip and
    the normalisation are applied to the cached bytes by the restatement's own code."""
    plain = {k: v for k, v in aug.items() if k != "flip"}
    tag = (key, repr(sorted(plain.items())))
    if key is None or tag not in _cache:
        u8 = np.stack([R.img_transform(f, plain) for f in frames.reshape((-1,) + frames.shape[-3:])])
        if key is not None:
            _cache[tag] = u8
    else:
        u8 = _cache[tag]
    if aug.get("flip", False):
        u8 = u8[:, :, ::-1]
    x = np.stack([R.normalise(i, norm["mean"], norm["std"], norm.get("to_rgb", True)) for i in u8]).astype(np.float16)
    return torch.from_numpy(np.concatenate([x, np.zeros(x.shape[:3] + (1,), np.float16)], -1))


def bits(t):
    return t.contiguous().view(torch.int16)


def assert_same_bits(got, want, what=""):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    same = torch.equal(bits(got), bits(want)) if got.dtype == torch.float16 else torch.equal(got, want)
    assert same, (what, int((got != want).sum()), "elements differ")


@pytest.mark.parametrize("to_rgb", [True, False])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("aug", [R50, R101], ids=["r50", "r101"])
def test_kernel_equals_restatement_full_size(aug, flip, to_rgb):
    frames = frames6()
    cfg = dict(aug, flip=flip)
    norm = dict(NORM, to_rgb=to_rgb)
    plan = P.ResamplePlan((900, 1600), cfg, norm)
    got = plan.run(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    assert got.shape == (6,) + plan.out_hw + (4,) and got.dtype == torch.float16
    assert not got[..., 3].any()
    assert_same_bits(got, expected(frames, cfg, norm, key="frames6"), (cfg, to_rgb))


@pytest.mark.parametrize("aug", [R50, R101], ids=["r50", "r101"])
def test_kernel_constant_frames(aug):
    """All-0 and all-255 frames: the resampled bytes are 0 / 255 (the coefficient rows sum to 2^22 up to their rounding,
    and the clamp takes the rest), through the table."""
    frames = np.zeros((2, 900, 1600, 3), np.uint8)
    frames[1] = 255
    plan = P.ResamplePlan((900, 1600), aug)
    got = plan.run(torch.from_numpy(frames).cuda())
    assert_same_bits(got, expected(frames, aug, NORM))


def test_kernel_eight_streams():
    """N = 48: the six images repeated for eight streams ([bs, cams, Hs, Ws, 3] input)."""
    frames = frames6()
    plan = P.ResamplePlan((900, 1600), R50).reserve(48, "cuda")
    tables = plan._dev["kx"].data_ptr()
    dev = torch.from_numpy(frames).cuda()[None].repeat(8, 1, 1, 1, 1).contiguous()
    got = plan.run(dev)
    assert got.shape == (48, 256, 704, 4)
    assert plan._dev["kx"].data_ptr() == tables   # resident: uploaded once ("cuda" and "cuda:0" are one device)
    want = expected(frames, R50, NORM, key="frames6")
    assert_same_bits(got, want.repeat(8, 1, 1, 1))


def test_kernel_golden_cases():
    """The reference's own ResizeCropFlipImage._img_transform (tests/golden/preprocess.npz) through the kernel: odd sizes
    (rows that are no multiple of 16 bytes, widths that are no multiple of 4), crop offsets on both axes, flip, enlargement."""
    n = 0
    for i, img, aug, want_u8 in golden_cases():
        plan = P.ResamplePlan(img.shape[:2], aug)
        got = plan.run(torch.from_numpy(img[None].copy()).cuda())
        x = R.normalise(want_u8, NORM["mean"], NORM["std"], True).astype(np.float16)
        want = torch.from_numpy(np.concatenate([x, np.zeros(x.shape[:2] + (1,), np.float16)], -1))[None]
        assert_same_bits(got, want, i)
        n += 1
    assert n >= 5


def test_equals_the_fp32_route():
    """Today's route: the host pipeline's fp32 NCHW tensor through simpb_image_to_nhwc4_f16 == the ingest's output."""
    from simpb_amd import _lib
    frames = frames6()
    x = torch.from_numpy(R.pipeline_nchw(frames, R50, NORM)).cuda()
    n, c, h, w = x.shape
    old = torch.empty(n, h, w, 4, dtype=torch.float16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    _lib.check(_lib.lib().simpb_image_to_nhwc4_f16(p(old), p(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), n, c, h, w,
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "image_to_nhwc4")
    new = P.ResamplePlan((900, 1600), R50).run(torch.from_numpy(frames).cuda())
    assert_same_bits(new, old)


def test_identity_configuration():
    """Source already 704 x 256, resize = 1: no resampling (as in Pillow), the table alone."""
    frames = np.random.RandomState(3).randint(0, 256, (6, 256, 704, 3)).astype(np.uint8)
    plan = P.ResamplePlan((256, 704), dict(resize=1))
    got = plan.run(torch.from_numpy(frames).cuda())
    lut = torch.from_numpy(plan.lut)
    t = torch.from_numpy(frames).long()
    want = torch.stack([lut[0][t[..., 2]], lut[1][t[..., 1]], lut[2][t[..., 0]], torch.zeros(t.shape[:-1], dtype=torch.float16)], -1)
    assert_same_bits(got, want)
    assert_same_bits(got, expected(frames, dict(resize=1), NORM))


def test_refused_call_leaves_the_output_untouched():
    from simpb_amd import _lib
    plan = P.ResamplePlan((90, 160), dict(resize=0.5)).reserve(1, "cuda")
    d = plan._dev
    src = torch.zeros(1, 90, 160, 3, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 45, 80, 4), 7.0, dtype=torch.float16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    ptrs = [p(out), p(src), p(d["mid"]), p(d["kx"]), p(d["xlo"]), p(d["xn"]), p(d["ky"]), p(d["ylo"]), p(d["yn"]), p(d["lut"])]
    good = [1, 90, 160, 45, 80, plan.taps_x, plan.taps_y, plan.src_row0, plan.src_rows, 0, 1]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = _lib.lib()
    for ints in (good[:5] + [65] + good[6:], good[:7] + [1, 90] + good[9:], [0] + good[1:], good[:4] + [4096] + good[5:]):
        assert h.simpb_preprocess_u8_nhwc4_f16(*ptrs, *ints, stream) == 1
    assert h.simpb_preprocess_u8_nhwc4_f16(*([ctypes.c_void_p(0)] + ptrs[1:]), *good, stream) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert h.simpb_preprocess_u8_nhwc4_f16(*ptrs, *good, stream) == 0    # (and the same buffers are taken when the arguments are right)
    torch.cuda.synchronize()
    assert_same_bits(out, expected(src.cpu().numpy(), dict(resize=0.5), NORM))


# ----------------------------------------------------------------------------------------------------------------- runners
def _model():
    from simpb_amd import configs, plugin
    cfg = configs.simpb_plus(anchor=synth.anchors(900))
    model = plugin.build_detector(cfg["model"]).eval()
    synth.load_procedural(model)
    model.cuda()
    model.fuse_conv_bn()
    model.half_backbone()
    return model


def _stream(frames, augs):
    """(raw u8 [1, 6, 900, 1600, 3], fp32 [1, 6, 3, 256, 704] of the restatement, metas) per frame; raw frames cycle over 3."""
    raws = [synth.raw_frames(1, f) for f in range(3)]
    out = []
    for f in range(frames):
        metas = synth.frame_metas(1, f)
        if augs[f] is not None:
            for m in metas["img_metas"]:
                m["aug_config"] = dict(augs[f])
        aug = metas["img_metas"][0]["aug_config"]
        tag = ("stream", f % 3, repr(sorted(aug.items())))
        if tag not in _cache:
            _cache[tag] = torch.from_numpy(R.pipeline_nchw(raws[f % 3].numpy(), aug, NORM))
        out.append((raws[f % 3], _cache[tag], metas))
    return out


def _same_result(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x) or isinstance(x, np.ndarray):
            x, y = torch.as_tensor(x), torch.as_tensor(y)
            assert x.shape == y.shape and torch.equal(x, y), (what, k)
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y)), (what, k)


def _run_pair(cls, stream, pinned, on_frame=None):
    """The same runner class twice: raw frames with raw_input, and the fp32 tensors of the restatement. Returns per frame
    (result, rec3d, rec2d) of both."""
    outs = []
    for raw_mode in (True, False):
        kw = dict(raw_input=(900, 1600)) if raw_mode else {}
        r = cls(_model(), 1, (256, 704), capacity=1536, device=torch.device("cuda"), use_graph=True, **kw)
        assert (r.img is None and r.raw is not None) if raw_mode else (r.raw is None)
        got = []
        for f, (raw, x, metas) in enumerate(stream):
            if on_frame is not None:
                on_frame(r, f, raw_mode)
            src = raw if raw_mode else x
            src = src.pin_memory() if pinned else src.cuda()
            res = r.step(src, metas)
            if res is not None:
                got.append((res[0]["img_bbox"], r.last_rec3d.clone(), r.last_rec2d.clone()))
        if hasattr(r, "flush"):
            res = r.flush()
            got.append((res[0]["img_bbox"], r.last_rec3d.clone(), r.last_rec2d.clone()))
        assert len(got) == len(stream)
        outs.append((got, r))
    return outs


def _compare(outs, name):
    (a, _), (b, _) = outs
    for f, ((ra, a3, a2), (rb, b3, b2)) in enumerate(zip(a, b)):
        assert torch.equal(a3, b3), (name, f, "rec3d")
        assert torch.equal(a2, b2), (name, f, "rec2d")
        _same_result(ra, rb, (name, f))


@pytest.mark.parametrize("name,frames,pinned", [("FrameRunner", 6, False), ("SplitPipelinedRunner", 10, True)])
def test_runner_raw_input_equals_fp32_input(name, frames, pinned):
    """The backbone sees identical f16 operands either way, so records and detections are equal bit for bit: cold frame,
    eager warm frames and replayed graphs (the ingest is the first node of the backbone graph)."""
    from simpb_amd import runner
    outs = _run_pair(getattr(runner, name), _stream(frames, [None] * frames), pinned)
    raw_runner, ref_runner = outs[0][1], outs[1][1]
    assert raw_runner.stats["replay"] >= 3 and raw_runner.stats == ref_runner.stats, (raw_runner.stats, ref_runner.stats)
    assert raw_runner.plan.key == P.plan_key((900, 1600), R50)
    _compare(outs, name)


@pytest.mark.parametrize("name,frames,switch", [("FrameRunner", 7, 4), ("SplitPipelinedRunner", 18, 10)])
def test_runner_follows_a_changed_aug_config(name, frames, switch):
    """The crop offset changes in the middle of a warm, replaying stream: the raw_input runner rebuilds its tables and
    drops its graphs by itself, and gives what the fp32 runner gives on the tensors of the new crop (the fp32 runner's
    graphs bake the decoder's crop in, so the test drops them by hand at that frame). Never the old crop."""
    from simpb_amd import runner
    new = dict(resize=0.44, crop=(0, 128, 704, 384))
    stream = _stream(frames, [None] * switch + [new] * (frames - switch))
    old_form = _cache[("stream", switch % 3, repr(sorted(R50.items())))]
    assert not torch.equal(stream[switch][1], old_form)   # the two crops do differ

    def on_frame(r, f, raw_mode):
        if f == switch and not raw_mode:
            torch.cuda.synchronize()
            r._drop_all_graphs()

    outs = _run_pair(getattr(runner, name), stream, name != "FrameRunner", on_frame)
    raw_runner, ref_runner = outs[0][1], outs[1][1]
    assert raw_runner.plan.crop == (0, 128, 704, 384)
    assert raw_runner.stats["replay"] >= 3 and raw_runner.stats == ref_runner.stats, (raw_runner.stats, ref_runner.stats)
    _compare(outs, name + " aug change")
    # a frame whose aug_config does not give the runner's image size is refused, not run
    bad = synth.frame_metas(1, frames)
    bad["img_metas"][0]["aug_config"] = dict(resize=0.44, crop=(0, 140, 704, 390))
    with pytest.raises(ValueError):
        raw_runner.step(stream[0][0].cuda(), bad)
    with pytest.raises(ValueError):
        raw_runner.step(stream[0][1].cuda(), stream[0][2])      # an fp32 tensor handed to a raw_input runner
