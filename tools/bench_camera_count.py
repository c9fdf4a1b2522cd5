"""What a camera costs: steady-state frames/s of rigs of N cameras, and the 3D aggregation of an N-camera frame in one launch
against the three launches it replaces. Synthetic inputs as bench.py's (synth.images / synth.frame_metas on the N-camera ring).

    python tools/bench_camera_count.py [--cams 4 5 6 7 8] [--rounds 5] [--steps 100] [--out FILE.json]

Three tables:
  1. the bs = 1 split runner (SplitPipelinedRunner, what `bench.py --gpus 1` times) at every N;
  2. the batch of independent streams (PipelinedRunner, `--bs 8`) at every N;
  3. the 3D aggregation alone at every N, on the operands of a bs = 1 frame (learned anchors, the model's own tokens):
     ONE launch (csrc/deform_agg_fused.hip, simpb_dfa_fused_forward_rig) against the THREE-launch route that already
     existed and takes any camera count (simpb_dfa_points_cams + simpb_dfa_weights_cams + the drop-in operator). The
     yardstick of the new code is that existing route, never the new code against itself. Both columns are device events
     around a run of back-to-back calls (the three launches have no timing id of their own, so neither column uses one),
     fp32 tokens for both; the f16-token form of the one launch, which a replayed frame runs, is a third column.

Protocol of tables 1 and 2: one runner per N (a rig is a property of the model), each in a FRESH CHILD PROCESS, one at a
time, so that no runner shares its process's streams and queues with another (`profiles/camera_count.md` has the figures that
asked for it). A child has a time limit (`--child-timeout`), and the tool stops at the first child that fails or runs out of
it. The runner is primed, then timed in `rounds` blocks: `--warmup` untimed steps in front of a block, `--steps` timed steps
between two device synchronisations, host clock. Reported per N: the median over the blocks and their spread (min .. max).
Frames/s per N is reported, not gated. The bar of table 3 is "one launch not slower
than three at any N"; the tool prints it and exits with status 1 if it is missed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build_model(num_cams, wh, bs, device):
    """bench.build_model at num_cams cameras (R50, procedural weights, fused conv + BN, fp16 backbone)."""
    from simpb_amd import configs, plugin, synth
    cfg = configs.simpb_plus(depth=50, input_shape=tuple(wh), anchor=synth.anchors(900), num_cams=num_cams)
    model = plugin.build_detector(cfg["model"]).eval()
    synth.load_procedural(model)
    model.to(device)
    model.fuse_conv_bn()
    model.half_backbone()
    with torch.no_grad():
        model.extract_feat(synth.images(bs, 0, tuple(wh), num_cams=num_cams).to(device))
    return model


class Rig:
    """One runner of an N-camera model with its ring of frames."""

    def __init__(self, runner, n, bs, wh):
        from simpb_amd import synth
        self.runner, self.n, self.bs, self.wh, self.frame = runner, n, bs, wh, 0
        self.imgs = [synth.images(bs, f % 4, wh, num_cams=n).to(runner.device) for f in range(4)]

    def step(self):
        from simpb_amd import synth
        f = self.frame
        self.frame += 1
        return self.runner.step(self.imgs[f % 4], synth.frame_metas(self.bs, f, self.wh, num_cams=self.n))


def time_rig(rig, args):
    """[ms/step per block] of one rig, alone on the device."""
    for _ in range(args.prime):
        rig.step()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(args.rounds):
        for _ in range(args.warmup):
            rig.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            rig.step()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) * 1e3 / args.steps)
    rig.runner.flush()
    return blocks


def row_of(rig, bs, b):
    med = statistics.median(b)
    return dict(cams=rig.n, ms_per_step=round(med, 4), min=round(min(b), 4), max=round(max(b), 4),
                spread_pct=round(100.0 * (max(b) - min(b)) / med, 2), frames_per_s=round(1e3 * bs / med, 1),
                blocks_ms=[round(x, 4) for x in b], stats=dict(rig.runner.stats), capacity=rig.runner.capacity)


def table(title, rows):
    print(f"\n{title}")
    print("| cameras | ms/step (median) | min .. max | spread | frames/s |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['cams']} | {r['ms_per_step']:.3f} | {r['min']:.3f} .. {r['max']:.3f} | {r['spread_pct']:.1f} % | {r['frames_per_s']:.0f} |")


def time_launches(model, n, wh, args):
    """The 3D aggregation of a bs = 1 frame at n cameras: one launch against three, `rounds` alternating blocks of `calls`
    back-to-back calls each between one event pair."""
    from simpb_amd import _lib, synth
    from simpb_amd.plugin import ops
    from simpb_amd.plugin.ops import _ptr as P, _stream
    lib = _lib.lib()
    dev = torch.device("cuda")
    head = model.head
    layer = next(l for op, l in zip(head.operation_order, head.layers) if op == "deformable")
    kps = layer.kps_generator
    with torch.no_grad():
        fm = model.extract_feat(synth.images(1, 0, wh, num_cams=n).to(dev))
        metas = synth.frame_metas(1, 0, wh, num_cams=n)
        proj, image_wh = metas["projection_mat"].to(dev).float().contiguous(), metas["image_wh"].to(dev).float().contiguous()
        anchor = head.instance_bank.anchor[None].float().contiguous()
        a = anchor.shape[1]
        feat = head.instance_bank.instance_feature[None] + torch.randn(1, a, layer.embed_dims, device=dev) * 0.1
        embed = head.anchor_encoder(anchor)
        learn = kps.learnable_fc(feat).contiguous()
        feat_logits = layer.weights_fc(feat + embed).contiguous()
        cam_embed = layer.camera_encoder(proj[:, :, :3].reshape(1, n, -1))
        cam_logits = torch.nn.functional.linear(cam_embed, layer.weights_fc.weight).contiguous()
        fix = kps.fix_scale.detach().float().contiguous()
        f32 = fm[0].float().contiguous()
        f16 = f32.half().contiguous()
        loc = torch.empty(1, a, layer.num_pts, n, 2, device=dev)
        w = torch.empty(1, a, layer.num_pts, n, layer.num_levels, layer.num_groups, device=dev)

        def one(tokens):
            return ops.dfa_fused(tokens, fm[1], fm[2], anchor, learn, fix, proj, image_wh, feat_logits, cam_logits, layer.num_groups)

        def three():
            _lib.check(lib.simpb_dfa_points_cams(P(loc), None, P(anchor), P(learn), P(fix), P(proj), P(image_wh), 1, a, fix.shape[0],
                                                 kps.num_learnable_pts, n, None, _stream()), "simpb_dfa_points_cams")
            _lib.check(lib.simpb_dfa_weights_cams(P(w), P(feat_logits), P(cam_logits), 1, a, n, layer.num_levels, layer.num_pts,
                                                  layer.num_groups, None, _stream()), "simpb_dfa_weights_cams")
            return ops.deformable_aggregation_function(f32, fm[1], fm[2], loc, w)

        routes = dict(three_launches_f32=three, one_launch_f32=lambda: one(f32), one_launch_f16=lambda: one(f16))
        want = three().reshape(1, a, -1)
        err, scale = float((routes["one_launch_f32"]() - want).abs().max()), float(want.abs().max())
        blocks = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                for _ in range(8):
                    fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                blocks[k].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    row = dict(cams=n, anchors=a, tokens_per_camera=int(fm[0].shape[1]) // n, one_vs_three_max_abs_diff=err,
               three_max_abs=scale)
    for k, b in blocks.items():
        row[k + "_us"] = round(statistics.median(b), 2)
        row[k + "_us_min_max"] = [round(min(b), 2), round(max(b), 2)]
    row["one_not_slower"] = row["one_launch_f32_us"] <= row["three_launches_f32_us"]
    return row


def measure(args):
    """--one KIND N: one measurement in this process, its row as one JSON line on stdout."""
    from simpb_amd.runner import PipelinedRunner, SplitPipelinedRunner
    kind, n = args.one[0], int(args.one[1])
    device = torch.device("cuda")
    torch.set_num_threads(max(1, min(4, len(os.sched_getaffinity(0)))))
    torch.backends.cudnn.benchmark = True
    wh = tuple(args.image_wh)
    if kind == "launches":
        row = time_launches(build_model(n, wh, 1, device), n, wh, args)
    else:
        bs = 1 if kind == "split_bs1" else args.bs
        cls = SplitPipelinedRunner if kind == "split_bs1" else PipelinedRunner
        rig = Rig(cls(build_model(n, wh, bs, device), bs, (wh[1], wh[0]), capacity=args.capacity, device=device, use_graph=True,
                      independent_streams=bs > 1), n, bs, wh)
        row = row_of(rig, bs, time_rig(rig, args))
    row["device"] = torch.cuda.get_device_name(0)
    print("ROW " + json.dumps(row), flush=True)


def child(args, kind, n):
    """A fresh process per measurement (see the protocol above); the parent never opens the device."""
    cmd = [sys.executable, os.path.abspath(__file__), "--one", kind, str(n), "--bs", str(args.bs), "--rounds", str(args.rounds),
           "--steps", str(args.steps), "--calls", str(args.calls), "--warmup", str(args.warmup), "--prime", str(args.prime),
           "--capacity", str(args.capacity), "--image-wh", str(args.image_wh[0]), str(args.image_wh[1])]
    try:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"{kind} at {n} cameras did not finish within {args.child_timeout} s: stopping")
    rows = [line[4:] for line in done.stdout.splitlines() if line.startswith("ROW ")]
    if done.returncode != 0 or not rows:
        raise SystemExit(f"{kind} at {n} cameras ended with status {done.returncode}")
    return json.loads(rows[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, nargs="+", default=[4, 5, 6, 7, 8])
    ap.add_argument("--bs", type=int, default=8, help="streams of table 2 (0: skip it)")
    ap.add_argument("--skip-bs1", action="store_true", help="skip table 1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls per block of table 3")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--prime", type=int, default=10)
    ap.add_argument("--capacity", type=int, default=1536)
    ap.add_argument("--image-wh", type=int, nargs=2, default=(704, 256))
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    ap.add_argument("--child-timeout", type=float, default=300.0, help="seconds one measurement (one child process) may take")
    ap.add_argument("--one", nargs=2, metavar=("KIND", "N"), default=None, help="(internal) one measurement in this process")
    args = ap.parse_args()
    if args.one is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_camera_count.py measures on the GPU; there is none here")
        return measure(args)
    result = dict(tool="bench_camera_count", image_wh=list(args.image_wh), capacity=args.capacity, rounds=args.rounds,
                  steps_per_block=args.steps, calls_per_block=args.calls, warmup=args.warmup)
    result["launches"] = [child(args, "launches", n) for n in args.cams]
    result["device"] = result["launches"][0]["device"]
    if not args.skip_bs1:
        result["split_bs1"] = [child(args, "split_bs1", n) for n in args.cams]
        table("bs = 1, SplitPipelinedRunner", result["split_bs1"])
    if args.bs > 0:
        result["batch"] = [child(args, "batch", n) for n in args.cams]
        table(f"bs = {args.bs}, PipelinedRunner, independent streams", result["batch"])

    print("\nthe 3D aggregation of a bs = 1 frame alone, us per call (median of the blocks)")
    print("| cameras | three launches, f32 tokens | one launch, f32 tokens | one launch, f16 tokens | one not slower than three |")
    print("|---|---|---|---|---|")
    for r in result["launches"]:
        print(f"| {r['cams']} | {r['three_launches_f32_us']} | {r['one_launch_f32_us']} | {r['one_launch_f16_us']} | {r['one_not_slower']} |")
    result["one_not_slower_at_every_n"] = all(r["one_not_slower"] for r in result["launches"])
    if args.out:
        if os.path.dirname(args.out):
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))
    if not result["one_not_slower_at_every_n"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
