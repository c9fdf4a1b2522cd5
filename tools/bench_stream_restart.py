"""What a restarted stream costs: ms/step of a replayed frame of the batch of independent streams (PipelinedRunner, ResNet50
704x256, bs 8, synthetic inputs as `bench.py --bs 8`) in which 1 and 8 of the 8 streams restart, beside the ordinary warm
frame in the same process -- and beside what an operator had to do before `restart=` existed: build a new runner and run
its first frames until its graphs replay again.

    python tools/bench_stream_restart.py [--rounds 5] [--steps 100] [--out FILE.json]

Protocol: the runner is primed, its restart graphs are captured by one restart frame per feature slot (the one-off capture
cost: the wall time of those steps against an ordinary replayed step), every case is run once untimed. Then `rounds` rounds,
each timing every case in turn (alternating blocks: drift of the box hits all of them alike), `--warmup` untimed steps after
each switch, `--steps` timed steps between two device synchronisations, host clock. A timed block restarts its streams in
EVERY step: that is not a drive anybody has, it is the way to time one kind of frame in steady state. Reported per case: the
median over the rounds and the spread (min .. max) between its blocks. The rebuild: a second runner on the same model, timed
from its constructor to the synchronise behind the first step whose decoder AND backbone were replays, frames counted.
There is no pass mark: the numbers document what a restart costs."""
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
    ap.add_argument("--restarting", type=int, nargs="+", default=[0, 1, 8], help="streams that restart per step (0: the ordinary frame)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--prime", type=int, default=10)
    ap.add_argument("--capacity", type=int, default=1536)
    ap.add_argument("--image-wh", type=int, nargs=2, default=(704, 256))
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_restart.py measures on the GPU; there is none here")
    import bench
    from simpb_amd import synth
    from simpb_amd.runner import PipelinedRunner
    device = torch.device("cuda")
    torch.set_num_threads(max(1, min(4, len(os.sched_getaffinity(0)))))
    torch.backends.cudnn.benchmark = True
    wh = tuple(args.image_wh)
    model = bench.build_model(SimpleNamespace(depth=50, image_wh=wh, bs=args.bs, residual_damp=1.0, token_std=None), device)
    imgs = [synth.images(args.bs, f % 4, wh).to(device) for f in range(4)]

    def make():
        return PipelinedRunner(model, args.bs, (wh[1], wh[0]), capacity=args.capacity, device=device, use_graph=True,
                               independent_streams=True)

    runner = make()
    frame = [0]

    def step(k, r=None):
        f = frame[0]
        frame[0] += 1
        flags = None if not k else [i < k for i in range(args.bs)]
        return (r or runner).step(imgs[f % 4], synth.frame_metas(args.bs, f, wh), restart=flags)

    def timed(k, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for _ in range(args.prime):
        step(0)
    ordinary_ms = timed(0, 20)
    capture_ms = [timed(1, 1), timed(1, 1)]   # one restart frame per feature slot: each captures that slot's restart graph
    captured_stats = dict(runner.stats)
    for k in args.restarting:
        for _ in range(args.warmup):
            step(k)
    blocks = {k: [] for k in args.restarting}
    for _ in range(args.rounds):
        for k in args.restarting:
            for _ in range(args.warmup):
                step(k)
            blocks[k].append(timed(k, args.steps))
    runner.flush()
    stats = dict(runner.stats)

    # what it replaces: a new runner, until its steps are replays again
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fresh = make()
    frames = 0
    while True:
        before = fresh.stats["replay"]
        bb_ready = all(g is not None for g in fresh.bb_graph)
        step(0, fresh)
        frames += 1
        if (fresh.stats["replay"] > before and bb_ready) or frames >= 32:
            break
    fresh.flush()
    torch.cuda.synchronize()
    rebuild_ms = (time.perf_counter() - t0) * 1e3

    rows = []
    for k in args.restarting:
        b = blocks[k]
        med = statistics.median(b)
        rows.append(dict(restarting=k, of=args.bs, ms_per_step=round(med, 4), min=round(min(b), 4), max=round(max(b), 4),
                         spread_pct=round(100.0 * (max(b) - min(b)) / med, 2), blocks_ms=[round(x, 4) for x in b]))
    result = dict(tool="bench_stream_restart", device=torch.cuda.get_device_name(0), bs=args.bs, image_wh=list(wh),
                  capacity=runner.capacity, rounds=args.rounds, steps_per_block=args.steps, warmup_after_switch=args.warmup,
                  ordinary_ms_before_capture=round(ordinary_ms, 4), restart_graph_capture_steps_ms=[round(x, 3) for x in capture_ms],
                  stats_after_capture=captured_stats, stats=stats, rows=rows,
                  rebuild=dict(frames_until_replay=frames, ms=round(rebuild_ms, 2), stats=dict(fresh.stats)))
    if args.out:
        if os.path.dirname(args.out):
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print("| restarting | ms/step (median of %d blocks) | min .. max | spread |" % args.rounds)
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['restarting']} of {r['of']} | {r['ms_per_step']:.3f} | {r['min']:.3f} .. {r['max']:.3f} | {r['spread_pct']:.1f} % |")
    print(f"restart graph capture (two slots, one step each): {capture_ms[0]:.1f} ms, {capture_ms[1]:.1f} ms; "
          f"an ordinary replayed step just before: {ordinary_ms:.3f} ms")
    print(f"a new runner instead: {frames} frames, {rebuild_ms:.1f} ms until a step is all replays again")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
