"""What camera health costs (`camera_health=`, csrc/health.hip): the two launches alone, and frames/s with the feature on and
off. Reported, not gated.

    python tools/bench_camera_health.py [--steps 150] [--out FILE.json]

1. Each of the two launches alone: device events around 200 back-to-back calls, the median of five such blocks, at 6 and at
   48 images of 256 x 704. The statistics launch reads N * H * W * 8 bytes once; that count over its time is given as a
   fraction of the HBM peak (--hbm-peak, GB/s). In a frame the image is cache-resident right after the ingest wrote it, and in
   this loop the same images are read again and again (6 images are 8.6 MB, 48 are 69 MB, against a last-level cache of
   256 MB), so the figure is a rate out of cache, not an HBM measurement.
2. frames/s with camera_health on and off for the bs = 1 SplitPipelinedRunner and the bs = 8 PipelinedRunner of independent
   streams, raw u8 frames 1600 x 900 -> 704 x 256 staged on the device once, every camera healthy. Each of the four runs in a
   fresh process (profiles/camera_count.md: a second model in one process inherits the first one's allocator state): this
   tool starts itself again with --one. Host clock between two device synchronisations around --steps steps, after --prime
   and --warmup untimed ones; the median of --rounds such blocks."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SRC = (900, 1600)
AUG = dict(resize=0.44, crop=(0, 140, 704, 396))
WH = (704, 256)


def time_launches(args):
    from simpb_amd import health as H
    dev = torch.device("cuda")
    params = H.CameraHealth().params()
    rows = []
    for n in (6, 48):
        bs = n // 6
        images = torch.randn(n, WH[1], WH[0], 4, device=dev).half()
        partials = torch.empty(n, H.BANDS, H.PARTIAL_WORDS, dtype=torch.int64, device=dev)
        state = H.new_state(bs, 6, dev)
        cam_out = torch.empty(bs, 6, dtype=torch.uint8, device=dev)
        flags = torch.empty(bs, 6, dtype=torch.uint8, device=dev)
        calls = dict(stats=lambda: H.image_health_stats(images, out=partials),
                     verdict=lambda: H.camera_health_verdict(partials, state, params, (WH[1], WH[0]), cam_out=cam_out, flags=flags))
        row = dict(images=n, bytes_read=n * WH[0] * WH[1] * 8)
        for name, call in calls.items():
            for _ in range(20):
                call()
            blocks = []
            for _ in range(5):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200):
                    call()
                e1.record()
                torch.cuda.synchronize()
                blocks.append(e0.elapsed_time(e1) * 1e3 / 200)
            row[name + "_us"] = round(statistics.median(blocks), 3)
            row[name + "_us_blocks"] = [round(b, 3) for b in blocks]
        row["stats_gb_per_s"] = round(row["bytes_read"] / row["stats_us"] / 1e3, 1)
        row["stats_fraction_of_hbm_peak"] = round(row["stats_gb_per_s"] / args.hbm_peak, 3)
        rows.append(row)
    return rows


def time_runner(args):
    import bench
    from simpb_amd import synth
    from simpb_amd.runner import PipelinedRunner, SplitPipelinedRunner
    dev = torch.device("cuda")
    torch.set_num_threads(max(1, min(4, len(os.sched_getaffinity(0)))))
    torch.backends.cudnn.benchmark = True
    bs = 1 if args.one == "split" else 8
    model = bench.build_model(SimpleNamespace(depth=50, image_wh=WH, bs=bs, residual_damp=1.0, token_std=None), dev)
    kw = dict(camera_health=dict()) if args.health == "on" else {}
    if args.one == "split":
        runner = SplitPipelinedRunner(model, 1, (WH[1], WH[0]), capacity=args.capacity, device=dev, use_graph=True, raw_input=SRC, **kw)
    else:
        runner = PipelinedRunner(model, bs, (WH[1], WH[0]), capacity=args.capacity, device=dev, use_graph=True, raw_input=SRC,
                                 independent_streams=True, **kw)
    raws = [synth.raw_frames(bs, f, SRC).to(dev) for f in range(3)]
    frame = [0]

    def step():
        f = frame[0]
        frame[0] += 1
        metas = synth.frame_metas(bs, f, WH)
        for m in metas["img_metas"]:
            m["aug_config"] = dict(AUG)
        return runner.step(raws[f % 3], metas)

    for _ in range(args.prime):
        step()
    blocks = []
    for _ in range(args.rounds):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) * 1e3 / args.steps)
    runner.flush()
    med = statistics.median(blocks)
    out = dict(runner=args.one, bs=bs, camera_health=args.health, ms_per_step=round(med, 4), frames_per_s=round(1e3 * bs / med, 1),
               blocks_ms=[round(b, 4) for b in blocks], stats=dict(runner.stats))
    if args.health == "on":
        out["flags_seen"] = sorted({int(v) for v in runner.last_health.reshape(-1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--prime", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=1536)
    ap.add_argument("--hbm-peak", type=float, default=8000.0, help="GB/s the statistics launch's rate is set against")
    ap.add_argument("--parts", nargs="+", default=["launches", "split", "pipe8"], choices=["launches", "split", "pipe8"])
    ap.add_argument("--one", choices=["split", "pipe8"], default=None, help="(internal) time one runner in this process")
    ap.add_argument("--health", choices=["on", "off"], default="off")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera_health.py measures on the GPU; there is none here")
    if args.one is not None:
        print("RESULT " + json.dumps(time_runner(args)))
        return
    result = dict(tool="bench_camera_health", device=torch.cuda.get_device_name(0), image_wh=list(WH), steps_per_block=args.steps,
                  rounds=args.rounds, hbm_peak_gb_per_s=args.hbm_peak)
    if "launches" in args.parts:
        result["launches"] = time_launches(args)
        print("| images | statistics, us | GB/s (fraction of peak) | verdict, us |\n|---|---|---|---|")
        for r in result["launches"]:
            print(f"| {r['images']} | {r['stats_us']} | {r['stats_gb_per_s']} ({r['stats_fraction_of_hbm_peak']}) | {r['verdict_us']} |")
    result["runners"] = []
    for one in (p for p in args.parts if p != "launches"):
        for health in ("off", "on"):   # each in a fresh process
            cmd = [sys.executable, os.path.abspath(__file__), "--one", one, "--health", health, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--prime", str(args.prime), "--rounds", str(args.rounds), "--capacity", str(args.capacity)]
            run = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            line = next((l for l in run.stdout.splitlines() if l.startswith("RESULT ")), None)
            if run.returncode != 0 or line is None:
                raise SystemExit(f"{' '.join(cmd)} failed ({run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
            result["runners"].append(json.loads(line[len("RESULT "):]))
    if result["runners"]:
        print("| runner | camera_health | ms/step (median) | frames/s |\n|---|---|---|---|")
        for r in result["runners"]:
            print(f"| {r['runner']} (bs {r['bs']}) | {r['camera_health']} | {r['ms_per_step']} | {r['frames_per_s']} |")
    if args.out:
        if os.path.dirname(args.out):
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
