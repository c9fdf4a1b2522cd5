"""What a paused stream costs: steady-state ms/step of the batch of independent streams (PipelinedRunner, ResNet50 704x256,
bs 8, synthetic inputs as `bench.py --bs 8`) with 8, 6, 4 and 1 of the 8 streams active.

    python tools/bench_stream_activity.py [--rounds 5] [--steps 100] [--idle-images compute skip] [--out FILE.json]

Protocol: the runner is primed with every stream active, switched to its masked graphs by one paused frame, and every
occupancy is run once untimed (its shapes are the same, its 2D work is not). Then `rounds` rounds, each timing every
occupancy in turn (alternating blocks: drift of the box hits all of them alike), `--warmup` untimed steps after each switch,
`--steps` timed steps between two device synchronisations, host clock. Reported per occupancy: the median over the rounds and
the spread (min .. max) between its blocks. There is no pass mark: the numbers document what a pause costs.

An inactive stream still costs the 3D side of the decoder on its rows (static shapes) and, with idle_images="compute", the
backbone on its images; it costs no 2D slots (csrc/alloc.hip `active`). --idle-images compute skip builds one runner of each
kind and times them in alternating blocks (every occupancy of a round in one, then in the other): "8 of 8" of the "skip"
runner is what an all-live frame pays once the live-form graphs are in use. With "skip" the per-launch table of
tools/_image_skip.py is measured too (profiles/image_skip.md)."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--occupancy", type=int, nargs="+", default=[8, 6, 4, 1])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--prime", type=int, default=10)
    ap.add_argument("--capacity", type=int, default=1536)
    ap.add_argument("--image-wh", type=int, nargs=2, default=(704, 256))
    ap.add_argument("--idle-images", nargs="+", choices=["compute", "skip"], default=["compute"],
                    help="the runners' idle_images; both: one runner each, timed in alternating blocks")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_activity.py measures on the GPU; there is none here")
    import bench
    from simpb_amd import synth
    from simpb_amd.runner import PipelinedRunner
    device = torch.device("cuda")
    torch.set_num_threads(max(1, min(4, len(os.sched_getaffinity(0)))))
    torch.backends.cudnn.benchmark = True
    wh = tuple(args.image_wh)
    modes = list(dict.fromkeys(args.idle_images))
    runners = {}
    for mode in modes:
        model = bench.build_model(SimpleNamespace(depth=50, image_wh=wh, bs=args.bs, residual_damp=1.0, token_std=None), device)
        runners[mode] = PipelinedRunner(model, args.bs, (wh[1], wh[0]), capacity=args.capacity, device=device, use_graph=True,
                                        independent_streams=True, idle_images=mode)
    imgs = [synth.images(args.bs, f % 4, wh).to(device) for f in range(4)]
    frame = {mode: 0 for mode in modes}

    def step(mode, k):
        f = frame[mode]
        frame[mode] += 1
        mask = None if k is None else [i < k for i in range(args.bs)]
        return runners[mode].step(imgs[f % 4], synth.frame_metas(args.bs, f, wh), active=mask)

    for mode in modes:
        for _ in range(args.prime):
            step(mode, None)
        for k in args.occupancy:   # masked graphs captured, every occupancy seen once
            for _ in range(args.warmup):
                step(mode, k)
        runners[mode].flush()
    torch.cuda.synchronize()
    blocks = {(mode, k): [] for mode in modes for k in args.occupancy}
    for _ in range(args.rounds):
        for mode in modes:
            for k in args.occupancy:
                for _ in range(args.warmup):
                    step(mode, k)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(mode, k)
                torch.cuda.synchronize()
                blocks[mode, k].append((time.perf_counter() - t0) * 1e3 / args.steps)
            runners[mode].flush()   # (nothing of this runner in flight beside the other's blocks)
    rows = []
    for mode in modes:
        for k in args.occupancy:
            b = blocks[mode, k]
            med = statistics.median(b)
            rows.append(dict(idle_images=mode, active=k, of=args.bs, ms_per_step=round(med, 4), min=round(min(b), 4), max=round(max(b), 4),
                             spread_pct=round(100.0 * (max(b) - min(b)) / med, 2), active_frames_per_s=round(1e3 * k / med, 1),
                             blocks_ms=[round(x, 4) for x in b]))
    result = dict(tool="bench_stream_activity", device=torch.cuda.get_device_name(0), bs=args.bs, image_wh=list(wh),
                  capacity=runners[modes[0]].capacity, rounds=args.rounds, steps_per_block=args.steps, warmup_after_switch=args.warmup,
                  stats={mode: dict(r.stats) for mode, r in runners.items()}, rows=rows)
    if "skip" in modes:
        del runners
        torch.cuda.empty_cache()
        import _image_skip
        result["launches"] = _image_skip.launch_table()
    if args.out:
        if os.path.dirname(args.out):
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print("| idle_images | active | ms/step (median of %d blocks) | min .. max | spread | frames/s of active streams |" % args.rounds)
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['idle_images']} | {r['active']} of {r['of']} | {r['ms_per_step']:.3f} | {r['min']:.3f} .. {r['max']:.3f} | "
              f"{r['spread_pct']:.1f} % | {r['active_frames_per_s']:.0f} |")
    if "launches" in result:
        _image_skip.print_launch_table(result["launches"])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
