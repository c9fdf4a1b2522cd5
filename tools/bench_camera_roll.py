"""Measures the per-camera mount roll of the camera frame ingest (csrc/preprocess.hip: resample_cols_lut_kernel<RollTable>) on the
GPU, beside the level pass it stands in for; one JSON line out. The workload is tools/bench_preprocess.py's: six 1600 x 900
NV12 cameras -> 704 x 256 (the R50 configuration).

  (a) `launch`: HIP-event time of the two ingest launches, warmed, --launches launches back to back between one pair of
      events, in --blocks alternating blocks of one run, for the level plan (no roll: the entry point and kernels of a build
      without this feature), a table of identity rows through the rolled kernel (the gather's own cost, with the level
      pass's memory traffic), 180 degrees and 3 degrees. The horizontal launch is the same in all four, so a difference
      between two lines is a difference of their vertical launches. The vertical launch ALONE is read from a kernel trace of
      the same loop (--profile: the forms once each, no events; run it under `rocprofv3 --kernel-trace --stats`).
  (b) `runner`: frames/s of SplitPipelinedRunner at bs = 1 on NV12 frames resident in HBM without raw_roll, with
      raw_roll=180 and with raw_roll=3 (every camera), alternated in blocks of one process. Same weights and pictures.

Each line carries its blocks and their spread (max - min): a difference below the spread of the lines it compares is noise.
A run that finds no GPU fails.

    python tools/bench_camera_roll.py [--launches 200] [--blocks 5] [--block-steps 40] [--skip-runner | --profile]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_preprocess import CONFIGS, build_model, nv12_frames  # noqa: E402

R50 = CONFIGS["r50_704x256"]
SRC = (900, 1600)


def launch_forms(torch):
    """{name: (plan, frames)}: the six NV12 pictures through the level plan and three rolled ones."""
    from simpb_amd.preprocess import ROLL_IDENTITY, ResamplePlan
    six = nv12_frames(torch, 0)[0][0].cuda()
    plans = {"level": ResamplePlan(SRC, R50, frame_format="nv12"), "identity_rows": ResamplePlan(SRC, R50, frame_format="nv12", roll=1.0),
             "roll_180": ResamplePlan(SRC, R50, frame_format="nv12", roll=180.0), "roll_3": ResamplePlan(SRC, R50, frame_format="nv12", roll=3.0)}
    plans["identity_rows"].roll_ints = np.asarray([ROLL_IDENTITY], np.int32)   # (a plan never hands these over by itself: it goes level)
    for p in plans.values():
        p.reserve(6, "cuda")
    return {k: (p, six) for k, p in plans.items()}


def launch_leg(torch, args):
    forms = launch_forms(torch)
    dst = torch.empty(6, 256, 704, 4, dtype=torch.float16, device="cuda")
    go = {k: (lambda p=p, f=f: p.run(f, out=dst)) for k, (p, f) in forms.items()}
    go["level"]()
    ref = dst.clone()
    go["identity_rows"]()
    assert torch.equal(dst.view(torch.int16), ref.view(torch.int16))   # the identity rows give the level pass's bits
    if args.profile:
        for fn in go.values():
            for _ in range(args.launches):
                fn()
        torch.cuda.synchronize()
        return dict(profiled_launches_per_form=args.launches, forms=list(go))
    for fn in go.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    blocks = {k: [] for k in go}
    for _ in range(args.blocks):
        for name, fn in go.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            e1.synchronize()
            blocks[name].append(e0.elapsed_time(e1) / args.launches)
    out = {k: dict(ms=round(float(np.mean(v)), 5), block_ms=[round(x, 5) for x in v], spread_ms=round(max(v) - min(v), 5), images=6,
                   launches=args.launches * args.blocks) for k, v in blocks.items()}
    for k in ("identity_rows", "roll_180", "roll_3"):
        out[k + "_minus_level_ms"] = round(out[k]["ms"] - out["level"]["ms"], 5)
    out["level_spread_ms"] = out["level"]["spread_ms"]
    return out


def runner_leg(torch, args):
    from simpb_amd import synth
    from simpb_amd.runner import SplitPipelinedRunner
    ring = 4
    frames = [nv12_frames(torch, f)[0].cuda() for f in range(ring)]
    dev = torch.device("cuda")
    make = lambda **kw: SplitPipelinedRunner(build_model(torch), 1, (256, 704), capacity=1536, device=dev, use_graph=True,   # noqa: E731
                                             raw_input=SRC, raw_format="nv12", **kw)
    runners = {"no_roll": make(), "raw_roll_180": make(raw_roll=180.0), "raw_roll_3": make(raw_roll=3.0)}
    count = dict.fromkeys(runners, 0)

    def run(name, steps):
        for _ in range(steps):
            f = count[name]
            runners[name].step(frames[f % ring], synth.frame_metas(1, f))
            count[name] = f + 1

    for name in runners:   # cold frame, eager warm frames, graph capture: outside every timed block
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
                         spread_ms=round(max(ms) - min(ms), 4), timed_frames=args.blocks * args.block_steps, replays=runners[name].stats["replay"],
                         rolled_plan=bool(runners[name].plan.rolled))
    for k in ("raw_roll_180", "raw_roll_3"):
        out[k + "_minus_no_roll_ms"] = round(out[k]["ms_per_step"] - out["no_roll"]["ms_per_step"], 4)
    out["noise_ms"] = max(v["spread_ms"] for v in out.values() if isinstance(v, dict))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-steps", type=int, default=40)
    ap.add_argument("--skip-runner", action="store_true")
    ap.add_argument("--profile", action="store_true", help="the launch forms once each, untimed: the run for a kernel trace")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera_roll needs a GPU")
    out = dict(tool="bench_camera_roll", device=torch.cuda.get_device_name(0), launch=launch_leg(torch, args))
    if not (args.skip_runner or args.profile):
        out["runner"] = runner_leg(torch, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
