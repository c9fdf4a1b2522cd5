"""What moving a live stream costs (runner.StreamState, export_stream, step(..., adopt=); csrc/bank.hip
simpb_bank_export_stream / simpb_bank_import_stream), on the batch of independent streams (PipelinedRunner, ResNet50 704x256,
bs 8, synthetic inputs as `bench.py --bs 8`):

  1. the two launches alone, HIP events around `--launches` of each on the runner's own bank (600 x 256 floats per stream);
  2. ms/step of the runner with a stream exported from slot i and adopted into slot j every k-th step, beside the same
     runner without it, in alternating blocks;
  3. consolidation: 3 survivors of the bs-8 runner adopted into a fresh bs-4 runner (on a second copy of the model: a head's
     bank belongs to one runner) whose fourth slot starts cold, ms/step before and after.

    python tools/bench_stream_migrate.py [--rounds 5] [--steps 100] [--every 4] [--out FILE.json]

Protocol as tools/bench_stream_restart.py: the runner is primed, every case is run once untimed, then `rounds` rounds, each
timing every case in turn (alternating blocks: drift of the box hits all of them alike), `--warmup` untimed steps after each
switch, `--steps` timed steps between two device synchronisations, host clock; per case the median over the rounds and the
spread (min .. max) between its blocks. A state exported behind frame t is sealed when frame t's results come back, i.e.
inside step t + 1, so the adoption follows its export two steps later. There is no pass mark: the numbers document the cost."""
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
    ap.add_argument("--small-bs", type=int, default=4, help="batch size of the runner the survivors are consolidated into")
    ap.add_argument("--survivors", type=int, default=3)
    ap.add_argument("--every", type=int, default=4, help="a stream migrates every this many steps (case 2)")
    ap.add_argument("--slots", type=int, nargs=2, default=(1, 6), help="exported from slot i, adopted into slot j")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--prime", type=int, default=10)
    ap.add_argument("--capacity", type=int, default=1536)
    ap.add_argument("--image-wh", type=int, nargs=2, default=(704, 256))
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_migrate.py measures on the GPU; there is none here")
    import bench
    from simpb_amd import synth
    from simpb_amd.runner import PipelinedRunner
    device = torch.device("cuda")
    torch.set_num_threads(max(1, min(4, len(os.sched_getaffinity(0)))))
    torch.backends.cudnn.benchmark = True
    wh = tuple(args.image_wh)
    src_slot, dst_slot = args.slots

    def make(bs):
        model = bench.build_model(SimpleNamespace(depth=50, image_wh=wh, bs=bs, residual_damp=1.0, token_std=None), device)
        runner = PipelinedRunner(model, bs, (wh[1], wh[0]), capacity=args.capacity, device=device, use_graph=True,
                                 independent_streams=True)
        return runner, [synth.images(bs, f % 4, wh).to(device) for f in range(4)]

    runner, imgs = make(args.bs)
    frame = [0]
    pending = [None]   # the state exported last, waiting to be adopted

    def step(migrate):
        f = frame[0]
        frame[0] += 1
        metas = synth.frame_metas(args.bs, f, wh)
        adopt = None
        if migrate and f % args.every == 0 and pending[0] is not None and pending[0].sealed:
            # slot j goes on as the vehicle of slot i: its frame is that vehicle's from here on
            for k in ("projection_mat", "timestamp"):
                metas[k][dst_slot] = metas[k][src_slot]
            metas["img_metas"][dst_slot] = metas["img_metas"][src_slot]
            adopt, pending[0] = {dst_slot: pending[0]}, None
        out = runner.step(imgs[f % 4], metas, adopt=adopt)
        if migrate and f % args.every == args.every - 2:
            pending[0] = runner.export_stream(src_slot)
        return out

    def timed(migrate, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step(migrate)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for _ in range(args.prime):
        step(False)
    cases = (("no migration", False), (f"slot {src_slot} -> slot {dst_slot} every {args.every} steps", True))
    for _, m in cases:
        for _ in range(args.warmup + args.every):
            step(m)
    blocks = {name: [] for name, _ in cases}
    for _ in range(args.rounds):
        for name, m in cases:
            for _ in range(args.warmup):
                step(m)
            blocks[name].append(timed(m, args.steps))
    runner.flush()
    stats = dict(runner.stats)

    # 1. the launches alone
    bank = runner.head.instance_bank
    record = bank.export_stream(src_slot)
    launch_us = {}
    for name, call in (("export", lambda: bank.export_stream(src_slot, out=record)),
                       ("import", lambda: bank.import_stream(dst_slot, record, header=bank.record_dims()))):
        for _ in range(10):
            call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.launches):
            call()
        b.record()
        torch.cuda.synchronize()
        launch_us[name] = a.elapsed_time(b) * 1e3 / args.launches

    # 3. consolidation: the survivors go on in a smaller runner
    survivors = list(range(args.survivors))
    states = [runner.export_stream(s) for s in survivors]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    small, small_imgs = make(args.small_bs)
    build_ms = (time.perf_counter() - t0) * 1e3

    def small_step(adopt=None):
        f = frame[0]
        frame[0] += 1
        big = synth.frame_metas(args.bs, f, wh)   # the survivors keep their own poses and clocks
        metas = synth.frame_metas(args.small_bs, f, wh)
        for slot, s in enumerate(survivors):
            for k in ("projection_mat", "timestamp"):
                metas[k][slot] = big[k][s]
            metas["img_metas"][slot] = big["img_metas"][s]
        return small.step(small_imgs[f % 4], metas, adopt=adopt)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    small_step({slot: st for slot, st in enumerate(states)})
    frames = 1
    while frames < 32:
        before = small.stats["replay"]
        bb_ready = all(g is not None for g in small.bb_graph)
        small_step()
        frames += 1
        if small.stats["replay"] > before and bb_ready:
            break
    torch.cuda.synchronize()
    until_replay_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(args.warmup):
        small_step()
    small_blocks = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            small_step()
        torch.cuda.synchronize()
        small_blocks.append((time.perf_counter() - t0) * 1e3 / args.steps)
    small.flush()

    def row(name, b):
        med = statistics.median(b)
        return dict(case=name, ms_per_step=round(med, 4), min=round(min(b), 4), max=round(max(b), 4),
                    spread_pct=round(100.0 * (max(b) - min(b)) / med, 2), blocks_ms=[round(x, 4) for x in b])

    rows = [row(name, blocks[name]) for name, _ in cases]
    rows.append(row(f"bs {args.small_bs} with {args.survivors} adopted survivors", small_blocks))
    result = dict(tool="bench_stream_migrate", device=torch.cuda.get_device_name(0), bs=args.bs, image_wh=list(wh),
                  capacity=runner.capacity, rounds=args.rounds, steps_per_block=args.steps, warmup_after_switch=args.warmup,
                  every=args.every, slots=[src_slot, dst_slot], record_bytes=int(record.numel()),
                  launch_us={k: round(v, 3) for k, v in launch_us.items()}, launches=args.launches, stats=stats, rows=rows,
                  consolidation=dict(small_bs=args.small_bs, survivors=args.survivors, build_ms=round(build_ms, 1),
                                     frames_until_replay=frames, ms_until_replay=round(until_replay_ms, 1),
                                     stats=dict(small.stats)))
    if args.out:
        if os.path.dirname(args.out):
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(f"record: {record.numel()} bytes; export {launch_us['export']:.2f} us, import {launch_us['import']:.2f} us per launch "
          f"(HIP events over {args.launches} launches)")
    print("| case | ms/step (median of %d blocks) | min .. max | spread |" % args.rounds)
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['case']} | {r['ms_per_step']:.3f} | {r['min']:.3f} .. {r['max']:.3f} | {r['spread_pct']:.1f} % |")
    print(f"consolidation: new bs-{args.small_bs} runner built in {build_ms:.0f} ms, {frames} frames / {until_replay_ms:.0f} ms "
          "from the adoption frame until a step is all replays")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
