"""GPU: NV12 / NV21 frames through the ingest (csrc/preprocess.hip, simpb_preprocess_yuv420sp_nhwc4_f16). The expected value
is the existing restatement of the host pipeline applied to the witness's BGR, preprocess_ref.nhwc4_f16(yuv_ref.yuv420sp_to_bgr(
frame), aug, norm); the path is integer arithmetic plus a table, so every comparison is bit for bit. The runners' raw_format=
"nv12" is compared with the same runner class fed the witness's BGR frames. Every test does a fixed, small amount of work."""
import ctypes

import numpy as np
import pytest
import torch

from simpb_amd import preprocess as P
from simpb_amd import synth
from tests import preprocess_ref as R
from tests import yuv_ref as Y

pytestmark = pytest.mark.gpu

R50 = dict(resize=0.44, crop=(0, 140, 704, 396))
NORM = P.IMG_NORM_CFG
_cache = {}


def noise(n, hs, ws, seed):
    """Uniform-random planes: most triples are outside the RGB gamut, so all three clamps act at both ends."""
    return np.random.RandomState(seed).randint(0, 256, (n, hs * 3 // 2, ws)).astype(np.uint8)


def natural(hs, ws, frame=0, cams=6):
    """NV12 [cams, Hs * 3 / 2, Ws] of the synthetic generator's pictures."""
    return Y.bgr_to_nv12(synth.raw_frames(1, frame, src_hw=(hs, ws), num_cams=cams)[0].numpy())


def want(frames, aug, norm=NORM, standard="jfif", vu=0):
    return torch.from_numpy(R.nhwc4_f16(Y.yuv420sp_to_bgr(frames, standard, vu), aug, norm))


def same_bits(got, expected, what=""):
    got, expected = got.cpu(), expected.cpu()
    assert got.shape == expected.shape and got.dtype == expected.dtype == torch.float16, (what, got.shape, expected.shape)
    a, b = got.contiguous().view(torch.int16), expected.contiguous().view(torch.int16)
    assert torch.equal(a, b), (what, int((a != b).sum()), "elements differ")


def run(frames, hw, aug, norm=NORM, fmt="nv12", standard="jfif"):
    plan = P.ResamplePlan(hw, aug, norm, fmt, standard)
    out = plan.run(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    assert out.shape == (frames.shape[0],) + plan.out_hw + (4,) and not out[..., 3].any()
    return plan, out


# ------------------------------------------------------------------------------------------------------- small geometries
def test_half_size_noise_and_natural():
    """90 x 160 -> 45 x 80: rows of whole 16-byte chunks."""
    for frames in (noise(2, 90, 160, 1), natural(90, 160, cams=2)):
        _, got = run(frames, (90, 160), dict(resize=0.5))
        same_bits(got, want(frames, dict(resize=0.5)))
    bgr = Y.yuv420sp_to_bgr(noise(2, 90, 160, 1)).astype(np.int64)
    assert (bgr == 0).mean() > 0.05 and (bgr == 255).mean() > 0.05     # the clamps did act, at both ends


def test_rows_that_are_no_multiple_of_16_bytes():
    """62 x 100: the byte-load staging path; the output, 31 x 50, is no multiple of 4 wide either."""
    frames = noise(3, 62, 100, 2)
    plan, got = run(frames, (62, 100), dict(resize=0.5))
    assert plan.out_hw == (31, 50)
    same_bits(got, want(frames, dict(resize=0.5)))


@pytest.mark.parametrize("aug,first,last", [(dict(resize=0.5, crop=(0, 3, 48, 9)), 3, 20), (dict(resize=0.75, crop=(5, 3, 50, 8)), 2, 12)],
                         ids=["odd-first-row", "even-first-row"])
def test_crop_and_chroma_row_pairing(aug, first, last):
    """64 x 96 with a crop. Odd first needed source row: it takes the second half of a chroma pair whose first half is never
    read. Even first row: the first needed chroma row serves two needed luma rows; the last needed luma row (even) is the
    first of its pair. The second crop is 45 columns wide (no multiple of 4) and starts at column 5."""
    frames = noise(2, 64, 96, 3)
    plan, got = run(frames, (64, 96), aug)
    assert (plan.src_row0, plan.src_row0 + plan.src_rows - 1) == (first, last)
    same_bits(got, want(frames, aug))


def test_enlargement():
    frames = noise(2, 32, 48, 4)
    plan, got = run(frames, (32, 48), dict(resize=1.5))
    assert plan.out_hw == (48, 72)
    same_bits(got, want(frames, dict(resize=1.5)))


def test_identity_one_tap():
    """resize = 1: no resampling, so the output is the table applied to the converted pixels."""
    frames = noise(2, 32, 48, 5)
    plan, got = run(frames, (32, 48), dict(resize=1))
    assert plan.taps_x == plan.taps_y == 1
    bgr = torch.from_numpy(Y.yuv420sp_to_bgr(frames)).long()
    lut = torch.from_numpy(plan.lut)
    direct = torch.stack([lut[0][bgr[..., 2]], lut[1][bgr[..., 1]], lut[2][bgr[..., 0]], torch.zeros(bgr.shape[:-1], dtype=torch.float16)], -1)
    same_bits(got, direct)
    same_bits(got, want(frames, dict(resize=1)))


def test_output_width_no_multiple_of_four():
    aug = dict(resize=0.5, crop=(1, 0, 47, 32))     # 46 columns
    frames = noise(1, 64, 96, 6)
    plan, got = run(frames, (64, 96), aug)
    assert plan.out_hw[1] % 4 == 2
    same_bits(got, want(frames, aug))


# ------------------------------------------------------------------------------------------------------- parametrised
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("standard", ["jfif", "bt601", "bt709"])
@pytest.mark.parametrize("fmt", ["nv12", "nv21"])
@pytest.mark.parametrize("to_rgb", [True, False])
@pytest.mark.parametrize("flip", [False, True])
def test_options(flip, to_rgb, fmt, standard, n):
    frames = noise(n, 40, 64, 7)
    aug = dict(resize=0.5, flip=flip)
    norm = dict(NORM, to_rgb=to_rgb)
    _, got = run(frames, (40, 64), aug, norm, fmt, standard)
    same_bits(got, want(frames, aug, norm, standard, int(fmt == "nv21")), (flip, to_rgb, fmt, standard, n))


def test_chroma_order_matters():
    """The same bytes read as NV12 and as NV21 give different pictures (the option is not ignored), and NV21 of the swapped
    pairs gives NV12's picture."""
    frames = noise(2, 40, 64, 8)
    _, a = run(frames, (40, 64), dict(resize=0.5), fmt="nv12")
    _, b = run(frames, (40, 64), dict(resize=0.5), fmt="nv21")
    _, c = run(Y.to_nv21(frames), (40, 64), dict(resize=0.5), fmt="nv21")
    assert not torch.equal(a, b)
    same_bits(c, a)


@pytest.mark.parametrize("standard,triple,bgr", [("jfif", (0, 0, 0), None), ("jfif", (255, 255, 255), None),
                                                 ("bt601", (16, 128, 128), 0), ("bt601", (235, 128, 128), 255)])
def test_constant_planes(standard, triple, bgr):
    hs, ws = 40, 64
    frames = np.empty((1, hs * 3 // 2, ws), np.uint8)
    frames[:, :hs] = triple[0]
    frames[:, hs:, 0::2] = triple[1]
    frames[:, hs:, 1::2] = triple[2]
    if bgr is not None:     # limited-range black and white are BGR 0 and 255
        assert (Y.yuv420sp_to_bgr(frames, standard) == bgr).all()
    _, got = run(frames, (hs, ws), dict(resize=0.5), standard=standard)
    same_bits(got, want(frames, dict(resize=0.5), standard=standard))
    if bgr is not None:
        lut = torch.from_numpy(P.normalise_lut(NORM))[:, bgr]
        assert torch.equal(got[..., :3].cpu(), lut.expand(got.shape[:3] + (3,)))


# ------------------------------------------------------------------------------------------------------- full size, once
def full_size():
    """(NV12 u8 [6, 1350, 1600]: three cameras of the synthetic generator, three of uniform noise; expected f16 [6, 256, 704, 4])."""
    if "full" not in _cache:
        frames = np.ascontiguousarray(np.concatenate([natural(900, 1600, cams=3), noise(3, 900, 1600, 11)]))
        _cache["full"] = (frames, want(frames, R50))
    return _cache["full"]


def test_full_size_r50_six_and_forty_eight_images():
    frames, expected = full_size()
    plan = P.ResamplePlan((900, 1600), R50, frame_format="nv12")
    dev = torch.from_numpy(frames).cuda()
    same_bits(plan.run(dev), expected)
    got = plan.run(dev[None].repeat(8, 1, 1, 1).contiguous())      # [8, 6, 1350, 1600]
    assert got.shape == (48, 256, 704, 4)
    same_bits(got, expected.repeat(8, 1, 1, 1))


def test_same_result_as_the_bgr_route_on_the_device():
    for frames, hw, aug in ((full_size()[0], (900, 1600), R50), (noise(3, 62, 100, 12), (62, 100), dict(resize=0.5, flip=True))):
        bgr = torch.from_numpy(Y.yuv420sp_to_bgr(frames)).cuda()
        a = P.ResamplePlan(hw, aug).run(bgr)
        b = P.ResamplePlan(hw, aug, frame_format="nv12").run(torch.from_numpy(frames).cuda())
        same_bits(b, a)


def test_refused_call_leaves_the_output_untouched():
    from simpb_amd import _lib
    plan = P.ResamplePlan((90, 160), dict(resize=0.5), frame_format="nv12").reserve(1, "cuda")
    d = plan._dev
    frames = noise(1, 90, 160, 13)
    src = torch.from_numpy(frames).cuda()
    out = torch.full((1, 45, 80, 4), 7.0, dtype=torch.float16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    ptrs = [p(out), p(src), p(d["mid"]), p(d["kx"]), p(d["xlo"]), p(d["xn"]), p(d["ky"]), p(d["ylo"]), p(d["yn"]), p(d["lut"])]
    good = [1, 90, 160, 45, 80, plan.taps_x, plan.taps_y, plan.src_row0, plan.src_rows, 0, 1, 0] + list(plan.yuv)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = _lib.lib().simpb_preprocess_yuv420sp_nhwc4_f16

    def changed(i, v):
        return good[:i] + [v] + good[i + 1:]

    # odd height (with a row range that still fits), odd width, a chroma order of 2, iy = 0, too many taps, no images
    for ints in (changed(1, 91), changed(2, 161), changed(11, 2), changed(13, 0), changed(5, 65), changed(0, 0)):
        assert fn(*ptrs, *ints, stream) == 1, ints
    assert fn(*([ctypes.c_void_p(0)] + ptrs[1:]), *good, stream) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert fn(*ptrs, *good, stream) == 0     # (and the same buffers are taken when the arguments are right)
    torch.cuda.synchronize()
    same_bits(out, want(frames, dict(resize=0.5)))


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
    """(NV12 u8 [1, 6, 1350, 1600], the witness's BGR u8 [1, 6, 900, 1600, 3], metas) per frame; the pictures cycle over 3."""
    if "stream" not in _cache:
        nv = [natural(900, 1600, f)[None] for f in range(3)]
        _cache["stream"] = [(torch.from_numpy(x), torch.from_numpy(Y.yuv420sp_to_bgr(x))) for x in nv]
    out = []
    for f in range(frames):
        metas = synth.frame_metas(1, f)
        if augs[f] is not None:
            for m in metas["img_metas"]:
                m["aug_config"] = dict(augs[f])
        out.append(_cache["stream"][f % 3] + (metas,))
    return out


def _run_pair(cls, stream, pinned):
    """The same runner class twice: NV12 frames with raw_format="nv12", and the witness's BGR frames with raw_format="bgr".
    Returns per frame (result, rec3d, rec2d) of both, and the runners."""
    outs = []
    for fmt in ("nv12", "bgr"):
        r = cls(_model(), 1, (256, 704), capacity=1536, device=torch.device("cuda"), use_graph=True, raw_input=(900, 1600), raw_format=fmt)
        assert r.img is None and tuple(r.raw.shape) == ((1, 6, 1350, 1600) if fmt == "nv12" else (1, 6, 900, 1600, 3))
        got = []
        for nv, bgr, metas in stream:
            src = nv if fmt == "nv12" else bgr
            res = r.step(src.pin_memory() if pinned else src.cuda(), metas)
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
        assert ra.keys() == rb.keys(), (name, f)
        for k in ra:
            x, y = ra[k], rb[k]
            if torch.is_tensor(x) or isinstance(x, np.ndarray):
                x, y = torch.as_tensor(x), torch.as_tensor(y)
                assert x.shape == y.shape and torch.equal(x, y), (name, f, k)
            else:
                assert np.array_equal(np.asarray(x), np.asarray(y)), (name, f, k)


@pytest.mark.parametrize("name,frames,pinned", [("FrameRunner", 6, False), ("SplitPipelinedRunner", 10, True)])
def test_runner_nv12_equals_bgr(name, frames, pinned):
    """The backbone sees identical f16 operands either way, so device records and detections are equal bit for bit: cold
    frame, eager warm frames and replayed graphs (the ingest is the first node of the captured backbone graph)."""
    from simpb_amd import runner
    outs = _run_pair(getattr(runner, name), _stream(frames, [None] * frames), pinned)
    nv_runner, bgr_runner = outs[0][1], outs[1][1]
    assert nv_runner.stats["replay"] >= 3 and nv_runner.stats == bgr_runner.stats, (nv_runner.stats, bgr_runner.stats)
    assert nv_runner.plan.key == P.plan_key((900, 1600), R50, "nv12", "jfif") != bgr_runner.plan.key
    _compare(outs, name)
    # a frame of the wrong layout is refused before anything is enqueued
    before = dict(nv_runner.stats)
    stream = _stream(1, [None])
    for bad in (stream[0][1].cuda(), stream[0][0][..., :900, :].contiguous().cuda(), stream[0][0].float().cuda()):
        with pytest.raises(ValueError, match="nv12"):
            nv_runner.step(bad, stream[0][2])
    assert nv_runner.stats == before and getattr(nv_runner, "queue", []) == []
    with pytest.raises(ValueError):
        bgr_runner.step(stream[0][0].cuda(), stream[0][2])      # ... and an NV12 frame by a BGR runner
    # the detector refuses a frame that is not of the plan's layout, for both leading forms
    model = nv_runner.model
    for bad in (stream[0][1].cuda(), stream[0][1][0].cuda(), stream[0][0][0, :, :900].contiguous().cuda()):
        with pytest.raises(ValueError):
            model.extract_feat(bad, raw_plan=nv_runner.plan)


def test_runner_follows_a_changed_aug_config():
    """The crop offset changes in the middle of a warm, replaying NV12 stream: the plan is re-made (format and standard kept),
    the graphs are dropped and re-captured, and the results still match the BGR runner's, which does the same."""
    from simpb_amd import runner
    new = dict(resize=0.44, crop=(0, 128, 704, 384))
    outs = _run_pair(runner.FrameRunner, _stream(7, [None] * 4 + [new] * 3), False)
    nv_runner, bgr_runner = outs[0][1], outs[1][1]
    assert nv_runner.plan.crop == (0, 128, 704, 384) and nv_runner.plan.frame_format == "nv12"
    assert nv_runner.plan.key == P.plan_key((900, 1600), new, "nv12", "jfif")
    assert nv_runner.stats == bgr_runner.stats and nv_runner.stats["replay"] >= 3, (nv_runner.stats, bgr_runner.stats)
    _compare(outs, "FrameRunner aug change")


def test_runner_options_need_raw_input():
    from simpb_amd import runner
    model = _model()
    for kw in (dict(raw_format="nv12"), dict(raw_colour="bt709")):
        with pytest.raises(ValueError, match="raw_input"):
            runner.FrameRunner(model, 1, (256, 704), device=torch.device("cuda"), **kw)
    with pytest.raises(ValueError, match="frame format"):
        runner.FrameRunner(model, 1, (256, 704), device=torch.device("cuda"), raw_input=(900, 1600), raw_format="i420")
    with pytest.raises(ValueError, match="even"):
        runner.FrameRunner(model, 1, (256, 704), device=torch.device("cuda"), raw_input=(901, 1600), raw_format="nv12")
    r = runner.FrameRunner(model, 1, (256, 704), device=torch.device("cuda"), raw_input=(900, 1600), raw_format="nv21", raw_colour="bt709")
    assert tuple(r.raw.shape) == (1, 6, 1350, 1600) and (r.raw_format, r.raw_colour) == ("nv21", "bt709")
