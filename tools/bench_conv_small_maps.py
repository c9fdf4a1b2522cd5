"""The under-filled convolutions of ResNet50 stages 3-4 at 6 x 256 x 704, each shape on its own: the candidate tilings of
csrc/conv3x3.hip on the four 3x3 shapes (variants 1 and 4 are what variant 0 chose before the 64 x 64 staged forms existed),
and the staged tilings of the pointwise shapes with 1 024 and 2 048 input channels. Four rotating input buffers; an
event-timed loop of `reps` launches, repeated `rounds` times: the table shows the lowest and the highest round.
usage: python tools/bench_conv_small_maps.py [reps] [rounds]"""
import sys

import torch

sys.path.insert(0, ".")
from simpb_amd.plugin.ops import conv1x1_nhwc, conv3x3_nhwc, conv3x3_variant_for  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
NAMES3 = {1: "128x64 direct", 3: "32x64 direct K/4", 4: "64x64 direct K/4", 5: "128x64 staged", 7: "96x64 staged", 9: "64x64 staged",
          10: "64x64 staged K/2", 11: "64x64 staged K/4"}
NAMES1 = {2: "128x64", 3: "128x128", 4: "64x64"}
# (name, cin, cout, h, w, stride, launches per frame)
SHAPES3 = [("stage 3 stride 1", 256, 256, 16, 44, 1, 5), ("stage 3 stride 2", 256, 256, 32, 88, 2, 1),
           ("stage 4 stride 1", 512, 512, 8, 22, 1, 2), ("stage 4 stride 2", 512, 512, 16, 44, 2, 1)]
# (name, cin, cout, h, w, stride, launches per frame, residual read with 2x upsampling)
SHAPES1 = [("stage 3 conv1", 1024, 256, 16, 44, 1, 5, False), ("stage 4 conv1", 2048, 512, 8, 22, 1, 2, False),
           ("stage 4.0 conv1", 1024, 512, 16, 44, 1, 1, False), ("stage 4.0 downsample", 1024, 2048, 16, 44, 2, 1, False),
           ("FPN lateral 2", 1024, 256, 16, 44, 1, 1, True), ("FPN lateral 3", 2048, 256, 8, 22, 1, 1, False)]


def rounds_us(fn):
    for _ in range(10):
        fn(0)
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(REPS):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / REPS)
    return min(out), max(out)


def operands(cin, cout, h, w, k):
    xs = [torch.randn(6, cin, h, w, device="cuda", dtype=torch.half).contiguous(memory_format=torch.channels_last) for _ in range(4)]
    wt = (torch.randn(cout, cin, k, k, device="cuda", dtype=torch.half) * 0.02).contiguous(memory_format=torch.channels_last)
    return xs, wt, torch.randn(cout, device="cuda", dtype=torch.half)


for name, cin, cout, h, w, stride, count in SHAPES3:
    xs, wt, b = operands(cin, cout, h, w, 3)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    gflop = 2 * 6 * ho * wo * cout * 9 * cin / 1e9
    ref = conv3x3_nhwc(xs[0], wt, b, True, stride, variant=1).float()
    print(f"{name}: {cin}->{cout}, {6 * ho * wo} px, {gflop:.2f} GFLOP, x{count} per frame, variant 0 runs "
          f"{conv3x3_variant_for(6 * ho * wo, cin, cout)}", flush=True)
    for v, label in NAMES3.items():
        diff = float((conv3x3_nhwc(xs[0], wt, b, True, stride, variant=v).float() - ref).abs().max())
        lo, hi = rounds_us(lambda i: conv3x3_nhwc(xs[i & 3], wt, b, True, stride, variant=v))
        print(f"  v{v:<2d} {label:16s} {lo:6.1f} - {hi:6.1f} us  {gflop / lo * 1e3:4.0f} TFLOP/s  max |y - y(v1)| {diff:.1e}", flush=True)
for name, cin, cout, h, w, stride, count, up in SHAPES1:
    xs, wt, b = operands(cin, cout, h, w, 1)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    res = torch.randn(6, cout, ho // 2, wo // 2, device="cuda", dtype=torch.half).contiguous(memory_format=torch.channels_last) if up else None
    relu = not up
    ref = conv1x1_nhwc(xs[0], wt, b, res, relu, stride, up, variant=2).float()
    print(f"{name}: {cin}->{cout}, {6 * ho * wo} px, x{count} per frame", flush=True)
    for v, label in NAMES1.items():
        diff = float((conv1x1_nhwc(xs[0], wt, b, res, relu, stride, up, variant=v).float() - ref).abs().max())
        lo, hi = rounds_us(lambda i: conv1x1_nhwc(xs[i & 3], wt, b, res, relu, stride, up, variant=v))
        print(f"  v{v:<2d} {label:16s} {lo:6.1f} - {hi:6.1f} us  max |y - y(v2)| {diff:.1e}", flush=True)
