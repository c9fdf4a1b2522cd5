"""What a missing camera saves (and what the full rig pays for the mask existing): steady-state frames/s with cameras masked
(`step(..., cameras=)`), synthetic inputs as bench.py's.

    python tools/bench_camera_dropout.py [--rounds 5] [--steps 100] [--idle-images skip] [--out FILE.json]

Three tables:
  1. the bs = 1 split runner (SplitPipelinedRunner, what `bench.py --gpus 1` times) with 6 / 5 / 3 / 1 of the 6 cameras valid;
  2. the batch of independent streams (PipelinedRunner, `--bs 8`) with one camera down in 0 / 1 / 8 of the streams;
  3. the launches that know the mask, alone, at the masks of table 1 and the shapes of a bs = 1 frame: the fused 3D
     aggregation (csrc/deform_agg_fused.hip; event pairs recorded inside the C call around the launch, simpb_timing_*) and the
     three launches of the static allocation (csrc/alloc.hip; device events around a run of back-to-back calls: they have
     no timing id of their own).

Protocol of tables 1 and 2, as tools/bench_stream_activity.py: the runner is primed with the full rig, switched to its masked
graphs by one masked frame, every mask is run once untimed; then `rounds` rounds, each timing every mask in turn (alternating
blocks: drift of the box hits all of them alike), `--warmup` untimed steps after each switch, `--steps` timed steps between
two device synchronisations, host clock. Reported per mask: the median over the rounds and the spread (min .. max) between
its blocks. "6 valid" runs through the masked graphs with an all-ones mask: what the full rig costs once a camera has been
lost; the cost with `cameras=None` is bench.py's own number. There is no pass mark.

A masked camera still costs the ingest and, with --idle-images compute (the default), the backbone on its image slot; it
costs no 2D slots, no share of the 3D aggregation's gathers. --idle-images skip builds the runners of tables 1 and 2 with
idle_images="skip" and adds the per-launch table of tools/_image_skip.py (profiles/image_skip.md)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CAMS = 6


def first_valid(k):
    return [c < k for c in range(CAMS)]


def time_runner(runner, bs, wh, masks, args):
    """{label: [ms/step per block]} for the masks {label: cameras argument}."""
    from simpb_amd import synth
    device = runner.device
    imgs = [synth.images(bs, f % 4, wh).to(device) for f in range(4)]
    frame = [0]

    def step(cams):
        f = frame[0]
        frame[0] += 1
        return runner.step(imgs[f % 4], synth.frame_metas(bs, f, wh), cameras=cams)

    for _ in range(args.prime):
        step(None)
    for cams in masks.values():   # masked graphs captured, every mask seen once
        for _ in range(args.warmup):
            step(cams)
    torch.cuda.synchronize()
    blocks = {k: [] for k in masks}
    for _ in range(args.rounds):
        for label, cams in masks.items():
            for _ in range(args.warmup):
                step(cams)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(cams)
            torch.cuda.synchronize()
            blocks[label].append((time.perf_counter() - t0) * 1e3 / args.steps)
    runner.flush()
    return blocks


def rows_of(blocks, bs):
    rows = []
    for label, b in blocks.items():
        med = statistics.median(b)
        rows.append(dict(mask=label, ms_per_step=round(med, 4), min=round(min(b), 4), max=round(max(b), 4),
                         spread_pct=round(100.0 * (max(b) - min(b)) / med, 2), frames_per_s=round(1e3 * bs / med, 1),
                         blocks_ms=[round(x, 4) for x in b]))
    return rows


def table(title, rows):
    print(f"\n{title}")
    print("| mask | ms/step (median) | min .. max | spread | frames/s |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['mask']} | {r['ms_per_step']:.3f} | {r['min']:.3f} .. {r['max']:.3f} | {r['spread_pct']:.1f} % | {r['frames_per_s']:.0f} |")


def time_launches(model, wh, args):
    """The fused aggregation launch and the static allocation's three launches alone, per mask of table 1, on the operands of
    a bs = 1 frame (learned anchors, the model's own tokens)."""
    from simpb_amd import _lib, synth
    from simpb_amd.plugin import ops
    lib = _lib.lib()
    dev = torch.device("cuda")
    head = model.head
    layer = next(l for op, l in zip(head.operation_order, head.layers) if op == "deformable")
    alloc = next(l for op, l in zip(head.operation_order, head.layers) if op == "allocation")
    kps = layer.kps_generator
    n = 200
    with torch.no_grad():
        fm = model.extract_feat(synth.images(1, 0, wh).to(dev))
        metas = synth.frame_metas(1, 0, wh)
        proj, image_wh = metas["projection_mat"].to(dev).float().contiguous(), metas["image_wh"].to(dev).float().contiguous()
        anchor = head.instance_bank.anchor[None].float().contiguous()
        a = anchor.shape[1]
        feat = head.instance_bank.instance_feature[None] + torch.randn(1, a, layer.embed_dims, device=dev) * 0.1
        embed = head.anchor_encoder(anchor)
        learn = kps.learnable_fc(feat).contiguous()
        feat_logits = layer.weights_fc(feat + embed).contiguous()
        cam_embed = layer.camera_encoder(proj[:, :, :3].reshape(1, CAMS, -1))
        cam_logits = torch.nn.functional.linear(cam_embed, layer.weights_fc.weight).contiguous()
        tokens = getattr(fm[0], "simpb_f16", None) if head_reads_f16() else None
        tokens = fm[0] if tokens is None else tokens
        out = {}
        for k in args.valid:
            cam_valid = torch.tensor([first_valid(k)], dtype=torch.uint8, device=dev)
            # --- the aggregation: n launches, each between its own event pair
            _lib.check(lib.simpb_timing_enable(n + 8), "simpb_timing_enable")
            for _ in range(8):
                ops.dfa_fused(tokens, fm[1], fm[2], anchor, learn, kps.fix_scale, proj, image_wh, feat_logits, cam_logits,
                              layer.num_groups, cam_valid=cam_valid)
            lib.simpb_timing_reset()
            for _ in range(n):
                ops.dfa_fused(tokens, fm[1], fm[2], anchor, learn, kps.fix_scale, proj, image_wh, feat_logits, cam_logits,
                              layer.num_groups, cam_valid=cam_valid)
            buf = (ctypes.c_float * n)()
            got = lib.simpb_timing_read(1, buf, n)
            lib.simpb_timing_enable(0)
            daf = sorted(buf[i] * 1e3 for i in range(max(got, 0)))
            # --- the allocation: n calls (3 launches each) between one event pair
            m = dict(projection_mat=proj, image_wh=image_wh, image_wh_host=(int(wh[0]), int(wh[1])))
            for _ in range(8):
                alloc.allocate(anchor, m, capacity=args.capacity, cam_valid=cam_valid)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                alloc.allocate(anchor, m, capacity=args.capacity, cam_valid=cam_valid)
            e1.record()
            torch.cuda.synchronize()
            slots = int(alloc.last.group_start[CAMS])
            out[k] = dict(valid=k, daf_fused_us_median=round(daf[len(daf) // 2], 2) if daf else None,
                          daf_fused_us_min=round(daf[0], 2) if daf else None, launches=len(daf),
                          alloc_static_us_per_call=round(e0.elapsed_time(e1) * 1e3 / n, 2), slots_2d=slots,
                          tokens=str(tokens.dtype))
    return [out[k] for k in args.valid]


def head_reads_f16():
    from simpb_amd.plugin import routes
    return bool(routes.R.dfa_f16_tokens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8, help="streams of table 2 (0: skip it)")
    ap.add_argument("--valid", type=int, nargs="+", default=[6, 5, 3, 1], help="valid cameras of tables 1 and 3")
    ap.add_argument("--down-in", type=int, nargs="+", default=[0, 1, 8], help="streams with one camera down, table 2")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--prime", type=int, default=10)
    ap.add_argument("--capacity", type=int, default=1536)
    ap.add_argument("--image-wh", type=int, nargs=2, default=(704, 256))
    ap.add_argument("--idle-images", choices=["compute", "skip"], default="compute", help="the runners' idle_images")
    ap.add_argument("--tables", type=int, nargs="+", default=[1, 2, 3], help="which of the three tables to measure")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera_dropout.py measures on the GPU; there is none here")
    import bench
    from simpb_amd.runner import PipelinedRunner, SplitPipelinedRunner
    device = torch.device("cuda")
    torch.set_num_threads(max(1, min(4, len(os.sched_getaffinity(0)))))
    torch.backends.cudnn.benchmark = True
    wh = tuple(args.image_wh)
    build = lambda bs: bench.build_model(SimpleNamespace(depth=50, image_wh=wh, bs=bs, residual_damp=1.0, token_std=None), device)  # noqa: E731
    result = dict(tool="bench_camera_dropout", device=torch.cuda.get_device_name(0), image_wh=list(wh), capacity=args.capacity,
                  rounds=args.rounds, steps_per_block=args.steps, warmup_after_switch=args.warmup, idle_images=args.idle_images)

    model = build(1)
    result["launches"] = time_launches(model, wh, args) if 3 in args.tables else []
    if 1 in args.tables:
        runner = SplitPipelinedRunner(model, 1, (wh[1], wh[0]), capacity=args.capacity, device=device, use_graph=True,
                                      idle_images=args.idle_images)
        masks = {f"{k} of {CAMS} valid": [first_valid(k)] for k in args.valid}
        result["split_bs1"] = rows_of(time_runner(runner, 1, wh, masks, args), 1)
        result["split_bs1_stats"] = dict(runner.stats)
        table(f"bs = 1, SplitPipelinedRunner, idle_images={args.idle_images}", result["split_bs1"])
        del runner
    del model
    torch.cuda.empty_cache()

    if args.bs > 0 and 2 in args.tables:
        bs = args.bs
        model = build(bs)
        runner = PipelinedRunner(model, bs, (wh[1], wh[0]), capacity=args.capacity, device=device, use_graph=True,
                                 independent_streams=True, idle_images=args.idle_images)
        masks = {f"camera 1 down in {d} of {bs} streams": [[not (c == 1 and s < d) for c in range(CAMS)] for s in range(bs)]
                 for d in args.down_in if d <= bs}
        result["batch"] = rows_of(time_runner(runner, bs, wh, masks, args), bs)
        result["batch_stats"] = dict(runner.stats)
        table(f"bs = {bs}, PipelinedRunner, independent streams, idle_images={args.idle_images}", result["batch"])
        del runner, model
        torch.cuda.empty_cache()
    if args.idle_images == "skip":
        import _image_skip
        result["image_skip_launches"] = _image_skip.launch_table()
        _image_skip.print_launch_table(result["image_skip_launches"])

    print("\nthe launches alone (bs = 1 frame)")
    print("| valid cameras | fused aggregation, us (median / min) | static allocation, us per call (3 launches) | 2D slots |")
    print("|---|---|---|---|")
    for r in result["launches"]:
        print(f"| {r['valid']} | {r['daf_fused_us_median']} / {r['daf_fused_us_min']} | {r['alloc_static_us_per_call']} | {r['slots_2d']} |")
    if args.out:
        if os.path.dirname(args.out):
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
