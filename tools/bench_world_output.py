"""What the world record costs and what it saves (ResNet50 704x256, synthetic inputs as bench.py, bs 1 and bs 8):

  * host: ms per step of results.format_sample over the runner's results (all streams of the step), in tracking mode with
    threshold 0.2 and in detection mode without one, and of results.world_record_host on the same records;
  * device: the world-record launch alone (csrc/world.hip), `--launches` back-to-back launches between two device events;
  * runner: steady-state frames/s with world_output on and off -- two runners in one process, timed in alternating blocks
    (`--rounds` rounds of `--steps` steps between two device synchronisations, host clock), so drift of the box hits both
    alike; the spread between the blocks of the option OFF is the run-to-run spread the difference is read against.

    python tools/bench_world_output.py [--bs 1 8] [--rounds 5] [--steps 100] [--md profiles/world_output.md] [--out FILE.json]

bs 1 runs SplitPipelinedRunner, bs 8 PipelinedRunner with independent streams, as bench.py does. The runner with the option on
is built for detection mode without a threshold. There is no pass mark: the numbers document the cost."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CLASSES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
           "traffic_cone")


def metas_with_pose(bs, f, wh):
    """bench.py's synthetic metas plus the four pose entries: the stream's ego pose as ego -> global, a fixed lidar mount."""
    from simpb_amd import results, synth
    metas = synth.frame_metas(bs, f, wh)
    for s, m in enumerate(metas["img_metas"]):
        t = np.asarray(m["T_global"], np.float64)
        yaw = float(np.arctan2(t[1, 0], t[0, 0]))
        m.update(token=f"s{s}-f{f}", lidar2ego_rotation=results.yaw_quat(0.01).tolist(), lidar2ego_translation=[0.9, 0.0, 1.8],
                 ego2global_rotation=results.yaw_quat(yaw).tolist(), ego2global_translation=t[:3, 3].tolist())
    return metas


def measure(bs, args, device):
    import bench
    from simpb_amd import results
    from simpb_amd.runner import PipelinedRunner, SplitPipelinedRunner
    from simpb_amd import synth
    wh = tuple(args.image_wh)
    cls = SplitPipelinedRunner if bs == 1 else PipelinedRunner
    world_cfg = dict(classes=CLASSES, tracking=False, threshold=None)
    runners, frame = {}, {}
    for on in (False, True):
        model = bench.build_model(SimpleNamespace(depth=50, image_wh=wh, bs=bs, residual_damp=1.0, token_std=None), device)
        runners[on] = cls(model, bs, (wh[1], wh[0]), capacity=args.capacity, device=device, use_graph=True,
                          independent_streams=True, world_output=world_cfg if on else None)
        frame[on] = 0
    imgs = [synth.images(bs, f % 4, wh).to(device) for f in range(4)]
    metas = [metas_with_pose(bs, f, wh) for f in range(args.prime + 2 * args.rounds * (args.warmup + args.steps) + 8)]

    def step(on):
        f = frame[on]
        frame[on] += 1
        return runners[on].step(imgs[f % 4], metas[f % len(metas)])

    for on in (False, True):
        for _ in range(args.prime):
            step(on)
    torch.cuda.synchronize()
    blocks = {False: [], True: []}
    for _ in range(args.rounds):
        for on in (False, True):
            for _ in range(args.warmup):
                step(on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(on)
            torch.cuda.synchronize()
            blocks[on].append((time.perf_counter() - t0) * 1e3 / args.steps)
    # one more step with the option on: its results and records feed the host and launch timings
    res = step(True)
    f = frame[True] - 2   # (the pipelined runners return the frame before the one just fed)
    infos = metas[f % len(metas)]["img_metas"]
    r = runners[True]
    torch.cuda.synchronize()
    rec3d = r.last_rec3d.clone()
    k = rec3d.shape[1]
    host = {}
    for name, tracking, thr in (("tracking_thr0.2", True, 0.2), ("detection", False, None)):
        t0 = time.perf_counter()
        for _ in range(args.host_reps):
            kept = sum(len(results.format_sample(x["img_bbox"], i, CLASSES, tracking, thr)) for x, i in zip(res, infos))
        fs = (time.perf_counter() - t0) * 1e3 / args.host_reps
        tables = results.world_tables(CLASSES, tracking)
        rec_h, pose_h = rec3d.cpu().numpy(), np.stack([results.pose_row(i) for i in infos])
        t0 = time.perf_counter()
        for _ in range(args.host_reps):
            _, cnt = results.world_record_host(rec_h, pose_h, tables, thr)
        wh_ms = (time.perf_counter() - t0) * 1e3 / args.host_reps
        assert int(cnt.sum()) == kept, (int(cnt.sum()), kept)
        host[name] = dict(format_sample_ms_per_step=round(fs, 3), world_record_host_ms_per_step=round(wh_ms, 3),
                          boxes_kept_per_stream=round(kept / bs, 1), boxes_per_stream=k)
    # the launch alone
    pose = r.slot_inputs[0].dev["pose"]
    dec, cfg = r.head.decoder, r.world_output
    for _ in range(20):
        dec.world_record(rec3d, pose, None, cfg["tables"], cfg["threshold"])
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(args.launches):
        dec.world_record(rec3d, pose, None, cfg["tables"], cfg["threshold"])
    stop.record()
    stop.synchronize()
    launch_us = start.elapsed_time(stop) * 1e3 / args.launches
    for on in (False, True):
        runners[on].flush()
    out = dict(bs=bs, runner=cls.__name__, host=host, launch_us_back_to_back=round(launch_us, 2), launches=args.launches,
               readback_bytes_per_stream=k * 16 * 8 + 4, stats_off=runners[False].stats, stats_on=runners[True].stats)
    for on in (False, True):
        b = blocks[on]
        med = statistics.median(b)
        out["on" if on else "off"] = dict(ms_per_step=round(med, 4), min=round(min(b), 4), max=round(max(b), 4),
                                          spread_pct=round(100.0 * (max(b) - min(b)) / med, 2),
                                          frames_per_s=round(1e3 * bs / med, 1), blocks_ms=[round(x, 4) for x in b])
    out["drop_pct"] = round(100.0 * (out["on"]["ms_per_step"] / out["off"]["ms_per_step"] - 1.0), 2)
    out["drop_exceeds_off_spread"] = bool(out["drop_pct"] > out["off"]["spread_pct"])
    return out


def markdown(result):
    lines = ["# World record: measured cost", "",
             f"Measured by `tools/bench_world_output.py` on {result['device']} (host timings: that machine's CPU, "
             f"{result['host_threads']} torch threads), ResNet50 {result['image_wh'][0]}x{result['image_wh'][1]}, synthetic inputs, "
             f"{result['rounds']} rounds of {result['steps_per_block']} steps per setting in alternating blocks, median of the blocks; "
             "spread = (max - min) / median of a setting's own blocks.", "",
             "## Runner, option off against on (same process, same session)", "",
             "| bs | runner | off: ms/step (min .. max, spread) | on: ms/step (min .. max, spread) | frames/s off | frames/s on | "
             "cost of on | above the spread of off? |", "|---|---|---|---|---|---|---|---|"]
    for r in result["rows"]:
        a, b = r["off"], r["on"]
        lines.append(f"| {r['bs']} | {r['runner']} | {a['ms_per_step']:.3f} ({a['min']:.3f} .. {a['max']:.3f}, {a['spread_pct']:.1f} %) | "
                     f"{b['ms_per_step']:.3f} ({b['min']:.3f} .. {b['max']:.3f}, {b['spread_pct']:.1f} %) | {a['frames_per_s']:.0f} | "
                     f"{b['frames_per_s']:.0f} | {r['drop_pct']:+.2f} % ms/step | {'yes' if r['drop_exceeds_off_spread'] else 'no'} |")
    lines += ["", "## The launch alone", "",
              "| bs | us per launch (back-to-back launches between two device events, mean) | read-back added per stream |",
              "|---|---|---|"]
    for r in result["rows"]:
        lines.append(f"| {r['bs']} | {r['launch_us_back_to_back']:.2f} (of {r['launches']}) | {r['readback_bytes_per_stream']} B |")
    lines += ["", "## Host work per step it replaces (all streams of the step)", "",
              "| bs | mode | boxes kept per stream | format_sample ms/step | world_record_host ms/step |", "|---|---|---|---|---|"]
    for r in result["rows"]:
        for mode, h in r["host"].items():
            lines.append(f"| {r['bs']} | {mode} | {h['boxes_kept_per_stream']} of {h['boxes_per_stream']} | "
                         f"{h['format_sample_ms_per_step']:.3f} | {h['world_record_host_ms_per_step']:.3f} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--prime", type=int, default=10)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=1536)
    ap.add_argument("--image-wh", type=int, nargs=2, default=(704, 256))
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "world_output.md"), help="markdown report")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_world_output.py measures on the GPU; there is none here")
    device = torch.device("cuda")
    threads = max(1, min(4, len(os.sched_getaffinity(0))))
    torch.set_num_threads(threads)
    torch.backends.cudnn.benchmark = True
    rows = [measure(bs, args, device) for bs in args.bs]
    result = dict(tool="bench_world_output", device=torch.cuda.get_device_name(0), image_wh=list(args.image_wh), rounds=args.rounds,
                  steps_per_block=args.steps, warmup_after_switch=args.warmup, host_threads=threads, rows=rows)
    for path, text in ((args.out, json.dumps(result, indent=1)), (args.md, markdown(result))):
        if path:
            if os.path.dirname(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(text)
    print(markdown(result))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
