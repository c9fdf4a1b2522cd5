"""Measures the camera frame ingest (csrc/preprocess.hip, simpb_amd/preprocess.py) on the GPU; one JSON line out.

  (a) `kernel`: HIP-event time of the two ingest launches alone, warmed, --launches (>= 200) timed launches back to back
      between one pair of events, for the R50 configuration (1600 x 900 -> 704 x 396 -> crop to 704 x 256) and the derived
      R101 one (-> 1408 x 792 -> 1408 x 512), bs 1 and 8 (N = 6 and 48 images), for packed BGR frames and for the same
      pictures as NV12 (keys `..._nv12`), in the same run. Bytes are the ones the algorithm needs, computed from the plan:
      the needed source rows read once, the u8 intermediate written and read, the output written.
      Share of the bound = (bytes / HBM peak) / time; the peak is MI355X_MICROARCH.md's 8.0 TB/s spec figure (6.29 TB/s is
      what a float4 copy reaches there).
  (b) `runner`: frames/s of SplitPipelinedRunner at bs = 1 with these input forms in one process, alternated in blocks:
      fp32 frames resident in HBM (what bench.py times), fp32 frames in pinned host memory (bench.py --h2d, 13.0 MB per
      frame), raw u8 BGR frames in pinned host memory with the device ingest (25.9 MB per frame), NV12 frames in pinned
      host memory (13.0 MB per frame, raw_format="nv12"); plus raw and NV12 frames resident in HBM, which splits each
      raw form's cost into launches and copy. Same weights, and the same pictures: the BGR frames are the NV12 frames
      converted by the ingest's own rule, and the fp32 frames are the ingest's output widened to fp32, so every form
      decodes the same operands.
  (c) `cpu_pillow_ms`: the same preprocessing of one six-camera frame with Pillow + numpy on one CPU thread, if Pillow
      imports (a CPU number about CPU work).

  (d) `surface`: decoder surfaces (SurfaceLayout, simpb_preprocess_surface_nhwc4_f16) at R50 with 6 and 48 images.
      `launch`: the two ingest launches alone, timed as in (a), for tight NV12 (the existing entry point), NV12 at pitch 1792
      with 912 luma rows as one contiguous batch, the same surfaces as separate allocations behind the pointer table,
      tight P010 (twice the source bytes), and tight NV12 and BGR through the surface kernel beside their own kernels. `runner`: SplitPipelinedRunner frames/s with device-resident NV12 surfaces as a
      tight tensor, as a padded tensor (raw_layout) and as a pointer list (raw_surfaces) whose surfaces alternate between
      two pools -- the tensor forms pay the 13 / 14.5 MB device-to-device staging copy per frame, the pointer list 48 bytes.

  (e) `rig` (--only-rig; not part of a plain run): a rig of cameras that differ (RigPlan, simpb_preprocess_rig_nhwc4_f16).
      `launch`: the two ingest launches, --launches per block, in --blocks alternating blocks: the uniform six-camera rig
      (1600 x 900 NV12 at pitch 1792 -> 704 x 256) through the rig entry point and, as the yardstick, the same surfaces
      through simpb_preprocess_surface_nhwc4_f16 in pointer mode; and the mixed rig (three such cameras beside three 1920 x
      1080 P010 cameras at pitch 4096), which has no yardstick of equal work: the share of its horizontal workgroups that
      leave at once (the grid is padded to the tallest camera) stands beside it. `runner`: SplitPipelinedRunner frames/s
      with the uniform rig (raw_rig) beside the raw_surfaces runner on the same surface pools, in alternating blocks.

  (f) `planes` (--only-planes; not part of a plain run): the two ingest launches alone at R50 with 6 images for every frame
      format of the other producers (planar yuv420p / yvu420p, packed yuyv / uyvy, rgb, bgra, rgba: tight frames through
      simpb_preprocess_planes_nhwc4_f16) beside packed BGR and NV12 through their own entry points, --launches per block in
      --blocks alternating blocks of one run. All forms hold the same pictures and must give the same operand. The vertical
      launch is the same for every format, so a difference between two lines is a difference of their horizontal launches;
      `source_bytes_per_image` (ResamplePlan.bytes_per_image) says which existing format a new one should sit with.

  (g) `chroma` (--only-chroma; not part of a plain run): interpolated chroma (chroma="jpeg", libjpeg's upsampling) beside
      replicated chroma, six 1600 x 900 NV12 -> 704 x 256. `launch`: the two ingest launches, --launches per block in --blocks
      alternating blocks: replicated NV12 through its own tight kernel (the yardstick), through the surface kernel (the
      address-table form) and as a six-camera rig, then the same three with interpolated chroma (a tight batch takes the
      surface kernel), interpolated yuv420p and yuyv, and yuv444p. Every line carries a checksum of its operand (the int16
      bits summed in int64): the replicated lines must agree with each other and with the same lines of any other commit.
      `runner`: SplitPipelinedRunner frames/s on device-resident NV12 frames with raw_chroma off and on, in alternating blocks.
      --replicated-only leaves out every line that needs chroma=: the same tool then times a commit without the feature,
      for a comparison of the replicated launches in alternating processes on one box. --loop-jpeg N: nothing is timed, the
      interpolated tight NV12 ingest and the replicated one through the same surface kernel are launched N times each (the
      program to put behind `rocprofv3 --kernel-trace --stats --`: the trace splits each ingest into its two kernels).

A run that finds no GPU fails.

    python tools/bench_preprocess.py [--launches 200] [--blocks 5] [--block-steps 40]
                                     [--only-surface | --skip-surface | --only-rig | --only-planes | --only-chroma]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12       # bytes/s, spec (MI355X_MICROARCH.md, chip-level parameters)
HBM_COPY = 6.29e12      # bytes/s, measured float4 copy (same table)
CONFIGS = {"r50_704x256": dict(resize=0.44, crop=(0, 140, 704, 396)), "r101_1408x512": dict(resize=0.88, crop=(0, 280, 1408, 792))}


def nv12_frames(torch, frame_idx):
    """The synthetic generator's frame as NV12 u8 [1, 6, 1350, 1600] (JFIF forward transform, 2 x 2 chroma means, in fp32 on
    the device) and as the BGR u8 [1, 6, 900, 1600, 3] the ingest's own rule turns it into: the same picture in both forms."""
    from simpb_amd import synth
    from simpb_amd.preprocess import yuv_coefficients
    x = synth.raw_frames(1, frame_idx).cuda().float()
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    pool = lambda c: c.reshape(c.shape[:-2] + (450, 2, 800, 2)).mean(dim=(-3, -1))   # noqa: E731
    q = lambda v: (v + 0.5).floor().clamp(0, 255).to(torch.uint8)   # noqa: E731
    chroma = torch.stack([q(pool((b - y) / 1.772) + 128), q(pool((r - y) / 1.402) + 128)], -1)       # [1, 6, 450, 800, 2]
    nv12 = torch.cat([q(y), chroma.reshape(1, 6, 450, 1600)], dim=-2).contiguous()
    yoff, iy, irv, igu, igv, ibu = yuv_coefficients("jfif")
    up = lambda c: c.repeat_interleave(2, -2).repeat_interleave(2, -1).int() - 128   # noqa: E731
    c = iy * (nv12[..., :900, :].int() - yoff) + (1 << 15)
    cb, cr = up(chroma[..., 0]), up(chroma[..., 1])
    bgr = torch.stack([(c + ibu * cb) >> 16, (c + igu * cb + igv * cr) >> 16, (c + irv * cr) >> 16], -1).clamp(0, 255).to(torch.uint8)
    return nv12.cpu(), bgr.contiguous().cpu()


def kernel_leg(torch, args):
    from simpb_amd import _lib
    from simpb_amd.preprocess import ResamplePlan
    nv12, bgr = nv12_frames(torch, 0)
    out = {}
    for name, aug, fmt in [(n, a, f) for n, a in CONFIGS.items() for f in ("bgr", "nv12")]:
        plan = ResamplePlan((900, 1600), aug, frame_format=fmt)
        six = (bgr if fmt == "bgr" else nv12).cuda()
        pitch = int(_lib.lib().simpb_preprocess_mid_pitch(plan.out_hw[1]))
        per_image = plan.bytes_per_image(pitch)
        for bs in (1, 8):
            frames = six.repeat(bs, *([1] * (six.dim() - 1))).contiguous()
            n = bs * 6
            dst = torch.empty(n, *plan.out_hw, 4, dtype=torch.float16, device="cuda")
            plan.reserve(n, "cuda")
            for _ in range(20):
                plan.run(frames, out=dst)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                plan.run(frames, out=dst)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / args.launches
            nbytes = n * sum(per_image.values())
            floor_ms = nbytes / HBM_PEAK * 1e3
            out[f"{name}_bs{bs}" + ("" if fmt == "bgr" else "_" + fmt)] = dict(
                ms=round(ms, 5), images=n, launches=args.launches, bytes=nbytes, bytes_per_image=per_image,
                bytes_per_s=round(nbytes / (ms * 1e-3), 1), share_of_hbm_peak=round(floor_ms / ms, 4),
                share_of_measured_copy_rate=round(nbytes / HBM_COPY * 1e3 / ms, 4),
                bandwidth_bound=bool(floor_ms / ms >= 0.5),
                note="bound named bandwidth-bound when the algorithm's bytes at the HBM peak take at least half the measured time")
    return out


def build_model(torch):
    from simpb_amd import configs, plugin, synth
    cfg = configs.simpb_plus(anchor=synth.anchors(900))
    model = plugin.build_detector(cfg["model"]).eval()
    synth.load_procedural(model)
    model.cuda()
    model.fuse_conv_bn()
    model.half_backbone()
    return model


def runner_leg(torch, args):
    from simpb_amd import synth
    from simpb_amd.preprocess import ResamplePlan
    from simpb_amd.runner import SplitPipelinedRunner
    ring = 4
    pairs = [nv12_frames(torch, f) for f in range(ring)]
    nv12s, raws = [p[0] for p in pairs], [p[1] for p in pairs]
    plan = ResamplePlan((900, 1600), CONFIGS["r50_704x256"])
    # the fp32 form of the same pictures: the ingest's f16 operand widened (exact), as [1, 6, 3, 256, 704]
    fp32 = [plan.run(r.cuda())[..., :3].permute(0, 3, 1, 2).float().contiguous()[None] for r in raws]
    forms = {
        "fp32_hbm": dict(frames=fp32, raw=False, bytes_per_frame=0),
        "fp32_pinned_host": dict(frames=[x.cpu().pin_memory() for x in fp32], raw=False, bytes_per_frame=fp32[0].numel() * 4),
        "raw_u8_pinned_host": dict(frames=[r.pin_memory() for r in raws], raw=True, bytes_per_frame=raws[0].numel()),
        "nv12_pinned_host": dict(frames=[r.pin_memory() for r in nv12s], raw="nv12", bytes_per_frame=nv12s[0].numel()),
        # not deployment forms (a decoder's frames start on the host): raw frames resident in HBM, which split a raw
        # form's cost into the ingest launches (this minus fp32_hbm) and the copy (the pinned form minus this)
        "raw_u8_hbm": dict(frames=[r.cuda() for r in raws], raw=True, bytes_per_frame=0),
        "nv12_hbm": dict(frames=[r.cuda() for r in nv12s], raw="nv12", bytes_per_frame=0),
    }
    if args.profile_raw:   # the run for rocprofv3 --kernel-trace --stats: the raw form alone
        forms = {"raw_u8_pinned_host": forms["raw_u8_pinned_host"]}
    dev = torch.device("cuda")
    make = lambda **kw: SplitPipelinedRunner(build_model(torch), 1, (256, 704), capacity=1536, device=dev, use_graph=True, **kw)   # noqa: E731
    runners = {False: None if args.profile_raw else make(),
               True: make(raw_input=(900, 1600)),
               "nv12": None if args.profile_raw else make(raw_input=(900, 1600), raw_format="nv12")}
    count = {False: 0, True: 0, "nv12": 0}

    def run(form, steps):
        r = runners[form["raw"]]
        for _ in range(steps):
            f = count[form["raw"]]
            r.step(form["frames"][f % ring], synth.frame_metas(1, f))
            count[form["raw"]] = f + 1

    for form in forms.values():   # cold frame, eager warm frames, graph capture: outside every timed block
        run(form, 12)
    torch.cuda.synchronize()
    blocks = {k: [] for k in forms}
    for _ in range(args.blocks):
        for name, form in forms.items():
            run(form, 4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(form, args.block_steps)
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) / args.block_steps * 1e3)
    out = {}
    for name, ms in blocks.items():
        mean = float(np.mean(ms))
        out[name] = dict(ms_per_step=round(mean, 4), frames_per_s=round(1e3 / mean, 1), block_ms=[round(v, 4) for v in ms],
                         spread_ms=round(max(ms) - min(ms), 4), timed_frames=args.blocks * args.block_steps,
                         host_bytes_per_frame=forms[name]["bytes_per_frame"], replays=runners[forms[name]["raw"]].stats["replay"])
    if args.profile_raw:
        return out
    out["ingest_launches_ms"] = round(out["raw_u8_hbm"]["ms_per_step"] - out["fp32_hbm"]["ms_per_step"], 4)
    out["raw_copy_ms"] = round(out["raw_u8_pinned_host"]["ms_per_step"] - out["raw_u8_hbm"]["ms_per_step"], 4)
    out["fp32_copy_ms"] = round(out["fp32_pinned_host"]["ms_per_step"] - out["fp32_hbm"]["ms_per_step"], 4)
    out["raw_minus_fp32_pinned_ms"] = round(out["raw_u8_pinned_host"]["ms_per_step"] - out["fp32_pinned_host"]["ms_per_step"], 4)
    out["raw_minus_fp32_hbm_ms"] = round(out["raw_u8_pinned_host"]["ms_per_step"] - out["fp32_hbm"]["ms_per_step"], 4)
    out["nv12_ingest_launches_ms"] = round(out["nv12_hbm"]["ms_per_step"] - out["fp32_hbm"]["ms_per_step"], 4)
    out["nv12_copy_ms"] = round(out["nv12_pinned_host"]["ms_per_step"] - out["nv12_hbm"]["ms_per_step"], 4)
    out["nv12_minus_raw_pinned_ms"] = round(out["nv12_pinned_host"]["ms_per_step"] - out["raw_u8_pinned_host"]["ms_per_step"], 4)
    out["nv12_minus_fp32_pinned_ms"] = round(out["nv12_pinned_host"]["ms_per_step"] - out["fp32_pinned_host"]["ms_per_step"], 4)
    out["noise_ms"] = max(v["spread_ms"] for v in out.values() if isinstance(v, dict))   # the largest spread between blocks
    return out


PADDED = dict(pitch=1792, luma_rows=912)   # 1600 x 900 as a hardware decoder allocates it


def pack_nv12(torch, nv12, layout):
    """Tight NV12 u8 [..., 1350, 1600] -> surfaces u8 [..., image_bytes] of `layout` (pad bytes 0xFF)."""
    hs, ws = layout.src_hw
    out = torch.full(nv12.shape[:-2] + (layout.image_bytes,), 0xFF, dtype=torch.uint8)
    for r in range(hs):
        out[..., r * layout.pitch:r * layout.pitch + ws] = nv12[..., r, :]
    for i in range(hs // 2):
        off = layout.chroma_offset + i * layout.chroma_pitch
        out[..., off:off + ws] = nv12[..., hs + i, :]
    assert off + ws == layout.sample_end
    return out


def surface_launch_leg(torch, args):
    from simpb_amd import _lib
    from simpb_amd.preprocess import ResamplePlan, SurfaceLayout
    aug = CONFIGS["r50_704x256"]
    nv12, bgr = nv12_frames(torch, 0)
    six, six_bgr = nv12[0], bgr[0]                                 # [6, 1350, 1600], [6, 900, 1600, 3]
    layout = SurfaceLayout((900, 1600), "nv12", **PADDED)
    padded = pack_nv12(torch, six, layout)
    p010 = (six.to(torch.int16) << 8).view(torch.uint8).reshape(6, 1350, 3200)    # v << 8, little-endian words as bytes
    forms = {"nv12_tight": (ResamplePlan((900, 1600), aug, frame_format="nv12", colour="bt601"), six, False),
             "nv12_padded": (ResamplePlan((900, 1600), aug, frame_format="nv12", colour="bt601", layout=layout), padded, False),
             "nv12_padded_pointer_table": (ResamplePlan((900, 1600), aug, frame_format="nv12", colour="bt601", layout=layout), padded, True),
             "p010_tight": (ResamplePlan((900, 1600), aug, frame_format="p010", colour="bt601"), p010, False),
             # the tight forms through the surface kernel (a layout whose every field is spelled out takes the new entry point)
             # beside the kernels of the two older entry points: what those would cost as callers of the surface kernel
             "nv12_tight_surface_kernel": (ResamplePlan((900, 1600), aug, frame_format="nv12", colour="bt601",
                                                        layout=dict(image_bytes=1350 * 1600)), six.reshape(6, -1), False),
             "bgr_tight": (ResamplePlan((900, 1600), aug), six_bgr, False),
             "bgr_tight_surface_kernel": (ResamplePlan((900, 1600), aug, layout=dict(image_bytes=900 * 1600 * 3)), six_bgr.reshape(6, -1), False)}
    out = {}
    refs = {}
    for name, (plan, host, pointer) in forms.items():
        pitch = int(_lib.lib().simpb_preprocess_mid_pitch(plan.out_hw[1]))
        per_image = plan.bytes_per_image(pitch)
        for bs in (1, 8):
            n = bs * 6
            frames = host.cuda().repeat(bs, *([1] * (host.dim() - 1))).contiguous()
            dst = torch.empty(n, *plan.out_hw, 4, dtype=torch.float16, device="cuda")
            plan.reserve(n, "cuda")
            if pointer:   # one allocation per image; the table is written once, the launches read it
                singles = [frames[i].clone() for i in range(n)]
                table = torch.tensor(plan.surface_table(singles)[0], dtype=torch.int64, device="cuda")
                go = lambda: plan.run_table(table, out=dst)   # noqa: E731
            else:
                go = lambda: plan.run(frames, out=dst)   # noqa: E731
            for _ in range(20):
                go()
            torch.cuda.synchronize()
            ref = refs.setdefault(plan.frame_format == "bgr", dst[:6].clone())   # (the BGR pictures follow the jfif rule)
            assert torch.equal(dst[:6], ref), name        # every form decodes the same pictures to the same operand
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                go()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / args.launches
            nbytes = n * sum(per_image.values())
            out[f"{name}_bs{bs}"] = dict(ms=round(ms, 5), images=n, launches=args.launches, bytes=nbytes, source_bytes_per_image=per_image["source"],
                                         bytes_per_s=round(nbytes / (ms * 1e-3), 1), share_of_hbm_peak=round(nbytes / HBM_PEAK * 1e3 / ms, 4))
    for bs in (1, 8):
        t = out[f"nv12_tight_bs{bs}"]["ms"]
        for name in ("nv12_padded", "nv12_padded_pointer_table", "p010_tight"):
            out[f"{name}_bs{bs}"]["ms_minus_tight_nv12"] = round(out[f"{name}_bs{bs}"]["ms"] - t, 5)
        for name in ("nv12_tight", "bgr_tight"):
            out[f"{name}_surface_kernel_bs{bs}"]["ms_minus_older_kernel"] = round(out[f"{name}_surface_kernel_bs{bs}"]["ms"] - out[f"{name}_bs{bs}"]["ms"], 5)
    return out


def surface_runner_leg(torch, args):
    from simpb_amd import synth
    from simpb_amd.preprocess import SurfaceLayout
    from simpb_amd.runner import SplitPipelinedRunner
    ring = 4
    layout = SurfaceLayout((900, 1600), "nv12", **PADDED)
    tight = [nv12_frames(torch, f)[0] for f in range(ring)]
    padded = [pack_nv12(torch, x, layout) for x in tight]
    dev = torch.device("cuda")
    make = lambda **kw: SplitPipelinedRunner(build_model(torch), 1, (256, 704), capacity=1536, device=dev, use_graph=True,   # noqa: E731
                                             raw_input=(900, 1600), raw_format="nv12", **kw)
    # two surface pools of `ring` frames each, one allocation per camera: frame f reads pool f % 2 (a decoder hands out a
    # different surface every frame; the pictures are resident, as in the tensor forms, so only the form of delivery differs)
    pools = [[[padded[f][0, c].cuda().clone() for c in range(6)] for f in range(ring)] for _ in range(2)]
    forms = {"tight_tensor": dict(r=make(), feed=[x.cuda() for x in tight], copy_bytes=tight[0].numel()),
             "padded_tensor": dict(r=make(raw_layout=layout), feed=[x.cuda() for x in padded], copy_bytes=padded[0].numel()),
             "pointer_list": dict(r=make(raw_layout=layout, raw_surfaces=True), feed=None, copy_bytes=8 * 6)}
    count = dict.fromkeys(forms, 0)

    def run(name, steps):
        form = forms[name]
        for _ in range(steps):
            f = count[name]
            img = form["feed"][f % ring] if form["feed"] is not None else [pools[f % 2][f % ring]]
            form["r"].step(img, synth.frame_metas(1, f))
            count[name] = f + 1

    for name in forms:
        run(name, 12)
    torch.cuda.synchronize()
    blocks = {k: [] for k in forms}
    for _ in range(args.blocks):
        for name in forms:
            run(name, 4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.block_steps)
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) / args.block_steps * 1e3)
    out = {}
    for name, ms in blocks.items():
        mean = float(np.mean(ms))
        out[name] = dict(ms_per_step=round(mean, 4), frames_per_s=round(1e3 / mean, 1), block_ms=[round(v, 4) for v in ms],
                         spread_ms=round(max(ms) - min(ms), 4), timed_frames=args.blocks * args.block_steps,
                         device_copy_bytes_per_frame=forms[name]["copy_bytes"], replays=forms[name]["r"].stats["replay"])
    out["pointer_minus_padded_tensor_ms"] = round(out["pointer_list"]["ms_per_step"] - out["padded_tensor"]["ms_per_step"], 4)
    out["padded_minus_tight_tensor_ms"] = round(out["padded_tensor"]["ms_per_step"] - out["tight_tensor"]["ms_per_step"], 4)
    out["noise_ms"] = max(v["spread_ms"] for v in out.values() if isinstance(v, dict))
    return out


def rig_sources():
    """(uniform, mixed): six 1600 x 900 NV12 cameras on the padded layout; three of them beside three 1920 x 1080 P010 ones."""
    from simpb_amd.preprocess import CameraSource
    nus = CameraSource((900, 1600), CONFIGS["r50_704x256"], "nv12", layout=PADDED)
    hd = CameraSource((1080, 1920), dict(resize=0.44, crop=(70, 140, 774, 396)), "p010", "bt709", dict(pitch=4096, luma_rows=1088))
    return [nus] * 6, [nus] * 3 + [hd] * 3


def rig_launch_leg(torch, args):
    from simpb_amd.preprocess import RigPlan
    uniform, mixed = rig_sources()
    padded = pack_nv12(torch, nv12_frames(torch, 0)[0][0], uniform[0].surface)          # [6, image_bytes]
    gen = torch.Generator().manual_seed(0)
    out = {}
    for bs in (1, 8):
        n = bs * 6
        nus = [padded[i % 6].cuda().clone() for i in range(n)]
        # (integer arithmetic without a data-dependent branch: noise times like a picture)
        hd = [torch.randint(0, 256, (mixed[3].surface.image_bytes,), dtype=torch.uint8, generator=gen).cuda() for _ in range(n)]
        dst = torch.empty(n, 256, 704, 4, dtype=torch.float16, device="cuda")
        rig, alone, both = RigPlan(uniform).reserve(n, "cuda"), uniform[0].plan().reserve(n, "cuda"), RigPlan(mixed).reserve(n, "cuda")
        t_rig = torch.tensor(rig.surface_table(nus)[0], dtype=torch.int64, device="cuda")
        t_mixed = torch.tensor(both.surface_table([nus[i] if i % 6 < 3 else hd[i] for i in range(n)])[0], dtype=torch.int64, device="cuda")
        forms = {"uniform_rig": lambda: rig.run_table(t_rig, out=dst), "surface_pointer_table": lambda: alone.run_table(t_rig, out=dst),
                 "mixed_rig": lambda: both.run_table(t_mixed, out=dst)}
        alone.run_table(t_rig, out=dst)
        ref = dst.clone()
        rig.run_table(t_rig, out=dst)
        assert torch.equal(dst, ref)      # the yardstick and the rig decode the same pictures to the same operand
        blocks = {k: [] for k in forms}
        for go in forms.values():
            for _ in range(20):
                go()
        torch.cuda.synchronize()
        for _ in range(args.blocks):
            for name, go in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    go()
                e1.record()
                e1.synchronize()
                blocks[name].append(e0.elapsed_time(e1) / args.launches)
        res = {k: dict(ms=round(float(np.mean(v)), 5), block_ms=[round(x, 5) for x in v], spread_ms=round(max(v) - min(v), 5), images=n,
                       launches=args.launches * args.blocks) for k, v in blocks.items()}
        res["uniform_rig_minus_yardstick_ms"] = round(res["uniform_rig"]["ms"] - res["surface_pointer_table"]["ms"], 5)
        res["yardstick_spread_ms"] = res["surface_pointer_table"]["spread_ms"]
        rows = both.src_rows
        res["mixed_rig"]["src_rows"] = list(rows)
        res["mixed_rig"]["workgroups_leaving_early"] = round(1.0 - sum(rows) / (max(rows) * len(rows)), 5)
        res["uniform_rig"]["workgroups_leaving_early"] = 0.0
        out[f"bs{bs}"] = res
    return out


def rig_runner_leg(torch, args):
    from simpb_amd import synth
    from simpb_amd.runner import SplitPipelinedRunner
    ring = 4
    uniform, _ = rig_sources()
    layout = uniform[0].surface
    padded = [pack_nv12(torch, nv12_frames(torch, f)[0], layout) for f in range(ring)]
    dev = torch.device("cuda")
    make = lambda **kw: SplitPipelinedRunner(build_model(torch), 1, (256, 704), capacity=1536, device=dev, use_graph=True, **kw)   # noqa: E731
    pools = [[[padded[f][0, c].cuda().clone() for c in range(6)] for f in range(ring)] for _ in range(2)]
    runners = {"raw_surfaces": make(raw_input=(900, 1600), raw_format="nv12", raw_layout=layout, raw_surfaces=True),
               "uniform_rig": make(raw_rig=uniform)}
    count = dict.fromkeys(runners, 0)

    def run(name, steps):
        for _ in range(steps):
            f = count[name]
            runners[name].step([pools[f % 2][f % ring]], synth.frame_metas(1, f))
            count[name] = f + 1

    for name in runners:
        run(name, 12)
    torch.cuda.synchronize()
    blocks = {k: [] for k in runners}
    for _ in range(args.blocks):
        for name in runners:
            run(name, 4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.block_steps)
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) / args.block_steps * 1e3)
    out = {}
    for name, ms in blocks.items():
        mean = float(np.mean(ms))
        out[name] = dict(ms_per_step=round(mean, 4), frames_per_s=round(1e3 / mean, 1), block_ms=[round(v, 4) for v in ms],
                         spread_ms=round(max(ms) - min(ms), 4), timed_frames=args.blocks * args.block_steps, replays=runners[name].stats["replay"])
    out["rig_minus_raw_surfaces_ms"] = round(out["uniform_rig"]["ms_per_step"] - out["raw_surfaces"]["ms_per_step"], 4)
    return out


def plane_frames(torch, nv12, bgr):
    """The six pictures (NV12 u8 [6, 1350, 1600] and the BGR u8 [6, 900, 1600, 3] the ingest's rule makes of them) in every frame
    format, tight: 4:2:2 repeats each chroma row, the 4-byte formats carry alpha 255."""
    luma, pairs = nv12[:, :900], nv12[:, 900:].reshape(6, 450, 800, 2)
    cb, cr = pairs[..., 0], pairs[..., 1]
    planar = lambda a, b: torch.cat([luma.reshape(6, -1), a.reshape(6, -1), b.reshape(6, -1)], 1).reshape(6, 1350, 1600)   # noqa: E731
    y2, cb2, cr2 = luma.reshape(6, 900, 800, 2), cb.repeat_interleave(2, 1), cr.repeat_interleave(2, 1)
    yuyv = torch.stack([y2[..., 0], cb2, y2[..., 1], cr2], -1).reshape(6, 900, 1600, 2)
    alpha = torch.full((6, 900, 1600, 1), 255, dtype=torch.uint8)
    rgb = bgr.flip(-1)
    frames = dict(bgr=bgr, nv12=nv12, yuv420p=planar(cb, cr), yvu420p=planar(cr, cb), yuyv=yuyv, uyvy=yuyv.flip(-1), rgb=rgb,
                  bgra=torch.cat([bgr, alpha], -1), rgba=torch.cat([rgb, alpha], -1))
    return {k: v.contiguous() for k, v in frames.items()}


def planes_launch_leg(torch, args):
    from simpb_amd import _lib
    from simpb_amd.preprocess import ResamplePlan
    aug = CONFIGS["r50_704x256"]
    nv12, bgr = nv12_frames(torch, 0)
    forms = {}
    for fmt, host in plane_frames(torch, nv12[0], bgr[0]).items():
        plan = ResamplePlan((900, 1600), aug, frame_format=fmt).reserve(6, "cuda")
        forms[fmt] = (plan, host.cuda(), torch.empty(6, *plan.out_hw, 4, dtype=torch.float16, device="cuda"))
    ref = None
    for fmt, (plan, frames, dst) in forms.items():
        for _ in range(20):
            plan.run(frames, out=dst)
        torch.cuda.synchronize()
        ref = dst.clone() if ref is None else ref
        assert torch.equal(dst, ref), fmt        # every format holds the same pictures: the same operand
    blocks = {k: [] for k in forms}
    for _ in range(args.blocks):
        for fmt, (plan, frames, dst) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                plan.run(frames, out=dst)
            e1.record()
            e1.synchronize()
            blocks[fmt].append(e0.elapsed_time(e1) / args.launches)
    out = {}
    for fmt, v in blocks.items():
        plan = forms[fmt][0]
        per_image = plan.bytes_per_image(int(_lib.lib().simpb_preprocess_mid_pitch(plan.out_hw[1])))
        ms = float(np.mean(v))
        out[fmt] = dict(ms=round(ms, 5), block_ms=[round(x, 5) for x in v], spread_ms=round(max(v) - min(v), 5), images=6,
                        launches=args.launches * args.blocks, source_bytes_per_image=per_image["source"],
                        bytes_per_image=sum(per_image.values()), share_of_hbm_peak=round(6 * sum(per_image.values()) / HBM_PEAK * 1e3 / ms, 4))
    for fmt, v in out.items():
        v["ms_minus_bgr"] = round(v["ms"] - out["bgr"]["ms"], 5)
        v["ms_minus_nv12"] = round(v["ms"] - out["nv12"]["ms"], 5)
    return out


def chroma_forms(torch, args):
    """name -> (run(), out tensor): every launch form of leg (g), warmed."""
    from simpb_amd.preprocess import CameraSource, ResamplePlan, RigPlan
    aug = CONFIGS["r50_704x256"]
    nv12, bgr = nv12_frames(torch, 0)
    host = plane_frames(torch, nv12[0], bgr[0])
    luma, pairs = nv12[0][:, :900], nv12[0][:, 900:].reshape(6, 450, 800, 2)
    full = lambda c: c.repeat_interleave(2, 1).repeat_interleave(2, 2)   # noqa: E731
    host["yuv444p"] = torch.cat([luma, full(pairs[..., 0]), full(pairs[..., 1])], 1).contiguous()
    lines = [("nv12_replicated_tight", "nv12", {}, "batch"), ("nv12_replicated_surface", "nv12", {}, "table"),
             ("nv12_replicated_rig", "nv12", {}, "rig")]
    if not args.replicated_only:
        jpeg = dict(chroma="jpeg")
        lines += [("nv12_jpeg_tight", "nv12", jpeg, "batch"), ("nv12_jpeg_surface", "nv12", jpeg, "table"), ("nv12_jpeg_rig", "nv12", jpeg, "rig"),
                  ("yuv420p_jpeg", "yuv420p", jpeg, "batch"), ("yuyv_jpeg", "yuyv", jpeg, "batch"), ("yuv444p", "yuv444p", {}, "batch")]
    forms, keep = {}, []
    for name, fmt, kw, form in lines:
        frames = host[fmt].cuda()
        dst = torch.empty(6, 256, 704, 4, dtype=torch.float16, device="cuda")
        if form == "rig":
            plan = RigPlan([CameraSource((900, 1600), aug, fmt, **kw)] * 6)
            table = torch.tensor([frames[i].data_ptr() for i in range(6)], dtype=torch.int64, device="cuda")
            run = lambda plan=plan, table=table, dst=dst: plan.run_table(table, out=dst)   # noqa: E731
        else:
            plan = ResamplePlan((900, 1600), aug, frame_format=fmt, **kw).reserve(6, "cuda")
            if form == "table":
                table = torch.tensor([frames[i].data_ptr() for i in range(6)], dtype=torch.int64, device="cuda")
                run = lambda plan=plan, table=table, dst=dst: plan.run_table(table, out=dst)   # noqa: E731
            else:
                run = lambda plan=plan, frames=frames, dst=dst: plan.run(frames, out=dst)   # noqa: E731
        keep.append(frames)
        for _ in range(20):
            run()
        torch.cuda.synchronize()
        forms[name] = (run, dst, plan)
    return forms, keep


def chroma_launch_leg(torch, args):
    from simpb_amd import _lib
    forms, keep = chroma_forms(torch, args)
    blocks = {k: [] for k in forms}
    for _ in range(args.blocks):
        for name, (run, dst, plan) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                run()
            e1.record()
            e1.synchronize()
            blocks[name].append(e0.elapsed_time(e1) / args.launches)
    out = {}
    for name, v in blocks.items():
        run, dst, plan = forms[name]
        ms = float(np.mean(v))
        out[name] = dict(ms=round(ms, 5), block_ms=[round(x, 5) for x in v], spread_ms=round(max(v) - min(v), 5), images=6,
                         launches=args.launches * args.blocks, checksum=int(dst.view(torch.int16).to(torch.int64).sum()))
        if hasattr(plan, "bytes_per_image"):
            per_image = plan.bytes_per_image(int(_lib.lib().simpb_preprocess_mid_pitch(704)))
            out[name].update(source_bytes_per_image=per_image["source"], bytes_per_image=sum(per_image.values()))
    for name, v in out.items():
        v["ms_minus_replicated_tight"] = round(v["ms"] - out["nv12_replicated_tight"]["ms"], 5)
    same = {out[k]["checksum"] for k in out if "replicated" in k}
    assert len(same) == 1, "the replicated forms hold one operand"
    return out


def chroma_runner_leg(torch, args):
    from simpb_amd import synth
    from simpb_amd.runner import SplitPipelinedRunner
    ring = 4
    frames = [nv12_frames(torch, f)[0].cuda() for f in range(ring)]
    dev = torch.device("cuda")
    make = lambda **kw: SplitPipelinedRunner(build_model(torch), 1, (256, 704), capacity=1536, device=dev, use_graph=True,   # noqa: E731
                                             raw_input=(900, 1600), raw_format="nv12", **kw)
    runners = {"raw_chroma_off": make()}
    if not args.replicated_only:
        runners["raw_chroma_jpeg"] = make(raw_chroma="jpeg", raw_colour="jpeg")
    count = dict.fromkeys(runners, 0)

    def run(name, steps):
        for _ in range(steps):
            f = count[name]
            runners[name].step(frames[f % ring], synth.frame_metas(1, f))
            count[name] = f + 1

    for name in runners:
        run(name, 12)
    torch.cuda.synchronize()
    blocks = {k: [] for k in runners}
    for _ in range(args.blocks):
        for name in runners:
            run(name, 4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.block_steps)
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) / args.block_steps * 1e3)
    out = {}
    for name, ms in blocks.items():
        mean = float(np.mean(ms))
        out[name] = dict(ms_per_step=round(mean, 4), frames_per_s=round(1e3 / mean, 1), block_ms=[round(v, 4) for v in ms],
                         spread_ms=round(max(ms) - min(ms), 4), timed_frames=args.blocks * args.block_steps, replays=runners[name].stats["replay"])
    if "raw_chroma_jpeg" in out:
        out["jpeg_minus_off_ms"] = round(out["raw_chroma_jpeg"]["ms_per_step"] - out["raw_chroma_off"]["ms_per_step"], 4)
    return out


def cpu_leg(frames=3):
    try:
        from PIL import Image
    except ImportError:
        return None
    try:
        import torch
        torch.set_num_threads(1)
    except Exception:
        pass
    from simpb_amd import synth
    from simpb_amd.preprocess import IMG_NORM_CFG
    six = synth.raw_frames(1, 0)[0].numpy()
    mean = np.asarray(IMG_NORM_CFG["mean"], np.float32)
    stdinv = (1.0 / np.asarray(IMG_NORM_CFG["std"], np.float64)).astype(np.float32)
    times = []
    for _ in range(frames):
        t0 = time.perf_counter()
        for cam in six:
            img = np.asarray(Image.fromarray(cam).resize((704, 396)).crop((0, 140, 704, 396))).astype(np.float32)
            img = (img[..., ::-1] - mean) * stdinv
            np.ascontiguousarray(img.transpose(2, 0, 1))
        times.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_per_frame=round(float(np.median(times)), 2), frames=frames, threads=1, what="Pillow resize + crop, numpy normalise + "
                "transpose, six 1600 x 900 cameras; a CPU time of CPU work")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-steps", type=int, default=40)
    ap.add_argument("--skip-runner", action="store_true")
    ap.add_argument("--skip-surface", action="store_true", help="leave out the decoder-surface leg (d)")
    ap.add_argument("--only-surface", action="store_true", help="the decoder-surface leg (d) alone")
    ap.add_argument("--only-rig", action="store_true", help="the rig leg (e) alone")
    ap.add_argument("--only-planes", action="store_true", help="the frame-format leg (f) alone")
    ap.add_argument("--only-chroma", action="store_true", help="the interpolated-chroma leg (g) alone")
    ap.add_argument("--replicated-only", action="store_true", help="leg (g) without the lines that need chroma= (times any commit)")
    ap.add_argument("--loop-jpeg", type=int, default=0, help="leg (g): launch the interpolated tight NV12 ingest N times, time nothing")
    ap.add_argument("--profile-raw", action="store_true",
                    help="only the runner leg's raw form: the program to put behind `rocprofv3 --kernel-trace --stats --`")
    args = ap.parse_args()
    if args.launches < 200 or args.blocks * args.block_steps < 200:
        raise SystemExit("at least 200 timed launches and 200 timed frames per input form")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_preprocess.py needs a GPU: nothing here is measured on a CPU in its place")
    if args.only_rig:
        with torch.no_grad():
            rig = dict(launch=rig_launch_leg(torch, args), runner=None if args.skip_runner else rig_runner_leg(torch, args))
        print(json.dumps(dict(tool="bench_preprocess", device=torch.cuda.get_device_name(0), rig=rig)))
        return
    if args.only_chroma:
        with torch.no_grad():
            if args.loop_jpeg:
                forms, keep = chroma_forms(torch, args)
                for _ in range(args.loop_jpeg):
                    forms["nv12_jpeg_tight"][0]()
                    forms["nv12_replicated_surface"][0]()
                torch.cuda.synchronize()
                return
            chroma = dict(launch=chroma_launch_leg(torch, args), runner=None if args.skip_runner else chroma_runner_leg(torch, args))
        print(json.dumps(dict(tool="bench_preprocess", device=torch.cuda.get_device_name(0), chroma=chroma)))
        return
    if args.only_planes:
        with torch.no_grad():
            planes = dict(launch=planes_launch_leg(torch, args))
        print(json.dumps(dict(tool="bench_preprocess", device=torch.cuda.get_device_name(0), planes=planes)))
        return
    with torch.no_grad():
        surface = None
        if not (args.skip_surface or args.profile_raw):
            surface = dict(launch=surface_launch_leg(torch, args), runner=None if args.skip_runner else surface_runner_leg(torch, args))
        older = not args.only_surface
        result = dict(tool="bench_preprocess", device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK,
                      kernel=kernel_leg(torch, args) if older and not args.profile_raw else None,
                      runner=runner_leg(torch, args) if older and not args.skip_runner else None,
                      cpu_pillow=cpu_leg() if older and not args.profile_raw else None, surface=surface)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
