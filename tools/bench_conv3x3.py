"""csrc/conv3x3.hip, every tiling, against the vendor convolution + the in-place bias_act pass on the 3x3 shapes of
ResNet50 + FPN at 6 x 256 x 704 (and R101 1408 x 512 with --big). Rotates 4 input buffers so that the activations do not
stay in L2 between repetitions. usage: python tools/bench_conv3x3.py [--big]

--large-maps: the stride-1 launches on the large maps only (layer1 / layer2 conv2, FPN levels 0 and 1, and the FPN's group
launch), the staged form the tile rule chooses (7 or 8) against the resident variants 12 and 13 in one process: lowest and
highest of five rounds of 200 launches each, one JSON line per shape (profiles/conv3x3_large_maps.md). --only NAME[,NAME]
keeps the named shapes and --rounds R --reps N shortens the run (for a counter run of few kernels)."""
import json
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
import simpb_amd  # noqa: E402,F401  (vendor solver settings)
from simpb_amd.plugin.ops import bias_act_, conv3x3_nhwc  # noqa: E402

torch.backends.cudnn.benchmark = True


def timeit(fn, reps=30):
    for _ in range(5):
        fn(0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def rounds(fn):
    ts = [timeit(fn, arg("--reps", 200)) for _ in range(arg("--rounds", 5))]
    return round(min(ts), 2), round(max(ts), 2)


def large_maps(only):
    from simpb_amd.plugin.ops import conv3x3_group_tokens, conv3x3_resident_for, conv3x3_variant_for
    shapes = [("layer1 conv2", 64, 64, 64, 176), ("layer2 conv2", 128, 128, 32, 88), ("fpn 0", 256, 256, 64, 176), ("fpn 1", 256, 256, 32, 88)]
    for name, cin, cout, h, w in shapes:
        if only and name not in only:
            continue
        xs = [torch.randn(6, cin, h, w, device="cuda", dtype=torch.half).contiguous(memory_format=torch.channels_last) for _ in range(4)]
        wt = (torch.randn(cout, cin, 3, 3, device="cuda", dtype=torch.half) * 0.02).contiguous(memory_format=torch.channels_last)
        b = torch.randn(cout, device="cuda", dtype=torch.half)
        staged = conv3x3_variant_for(6 * h * w, cin, cout)
        want = conv3x3_nhwc(xs[0], wt, b, True, 1, variant=staged).view(torch.int16)
        out = {"shape": name, "cin": cin, "cout": cout, "hw": [h, w], "gflop": round(2 * 6 * h * w * cout * 9 * cin / 1e9, 2),
               "staged": staged, "variant0_resident": conv3x3_resident_for(6 * h * w, h, w, cin, cout), "us_low_high": {}, "same_bits": {}}
        for v in (staged, 12, 13):
            out["same_bits"][v] = bool(torch.equal(conv3x3_nhwc(xs[0], wt, b, True, 1, variant=v).view(torch.int16), want))
            out["us_low_high"][v] = rounds(lambda i: conv3x3_nhwc(xs[i & 3], wt, b, True, 1, variant=v))  # noqa: B023
        print(json.dumps(out), flush=True)
    if only and "fpn group" not in only:
        return
    hw = [(64, 176), (32, 88), (16, 44), (8, 22)]
    xs = [[torch.randn(6, 256, h, w, device="cuda", dtype=torch.half).contiguous(memory_format=torch.channels_last) for h, w in hw] for _ in range(4)]
    ws = [(torch.randn(256, 256, 3, 3, device="cuda", dtype=torch.half) * 0.02).contiguous(memory_format=torch.channels_last) for _ in hw]
    bs = [torch.randn(256, device="cuda", dtype=torch.half) for _ in hw]
    starts, at = [], 0
    for h, w in hw:
        starts.append(at)
        at += h * w
    col16 = torch.empty(1, 6 * at, 256, device="cuda", dtype=torch.half)
    out = {"shape": "fpn group", "gflop": round(sum(2 * 6 * h * w * 256 * 9 * 256 for h, w in hw) / 1e9, 2), "us_low_high": {}, "same_bits": {}}
    want = None
    for forms in ((8, 8, 8, 8), None, (13, 8, 8, 8), (13, 13, 8, 8), (13, 13, 13, 8), (13, 13, 13, 13)):
        conv3x3_group_tokens(xs[0], ws, bs, None, at, starts, col16=col16, variants=forms)
        got = col16.view(torch.int16).clone()
        want = got if want is None else want
        key = ",".join(map(str, forms)) if forms else "rule"
        out["same_bits"][key] = bool(torch.equal(got, want))
        out["us_low_high"][key] = rounds(lambda i: conv3x3_group_tokens(xs[i & 3], ws, bs, None, at, starts, col16=col16, variants=forms))  # noqa: B023
    print(json.dumps(out), flush=True)


if "--large-maps" in sys.argv:
    large_maps(arg("--only", "").split(",") if "--only" in sys.argv else None)
    sys.exit(0)

big = "--big" in sys.argv
H0, W0 = (128, 352) if big else (64, 176)
SHAPES = [("layer1 conv2", 64, 64, H0, W0, 1), ("layer2.0 conv2", 128, 128, H0, W0, 2), ("layer2 conv2", 128, 128, H0 // 2, W0 // 2, 1),
          ("layer3.0 conv2", 256, 256, H0 // 2, W0 // 2, 2), ("layer3 conv2", 256, 256, H0 // 4, W0 // 4, 1),
          ("layer4.0 conv2", 512, 512, H0 // 4, W0 // 4, 2), ("layer4 conv2", 512, 512, H0 // 8, W0 // 8, 1),
          ("fpn 0", 256, 256, H0, W0, 1), ("fpn 1", 256, 256, H0 // 2, W0 // 2, 1), ("fpn 2", 256, 256, H0 // 4, W0 // 4, 1),
          ("fpn 3", 256, 256, H0 // 8, W0 // 8, 1)]
total = {"vendor": 0.0, "auto": 0.0, "best": 0.0}
COUNT = {"layer1 conv2": 3, "layer2 conv2": 3, "layer3 conv2": 5, "layer4 conv2": 2}
for name, cin, cout, h, w, stride in SHAPES:
    xs = [torch.randn(6, cin, h, w, device="cuda", dtype=torch.half).contiguous(memory_format=torch.channels_last) for _ in range(4)]
    wt = (torch.randn(cout, cin, 3, 3, device="cuda", dtype=torch.half) * 0.02).contiguous(memory_format=torch.channels_last)
    b = torch.randn(cout, device="cuda", dtype=torch.half)
    vendor = lambda i: bias_act_(F.conv2d(xs[i & 3], wt, None, stride, 1), b, None, relu=True)  # noqa: E731
    ref = F.conv2d(xs[0].float(), wt.float(), b.float(), stride, 1).relu()
    ho, wo = ref.shape[2:]
    gflop = 2 * 6 * ho * wo * cout * 9 * cin / 1e9
    tv = timeit(vendor)
    line = f"{name:15s} {cin:3d}->{cout:3d} {h:3d}x{w:3d} s{stride} {gflop:5.2f} GF  vendor+bias_act {tv:6.1f} us |"
    best = 1e9
    for v in range(14):
        if v >= 12 and (stride != 1 or cin not in (64, 128, 256)):   # the resident form: SIMPB_EINVAL on these
            continue
        fn = lambda i: conv3x3_nhwc(xs[i & 3], wt, b, True, stride, variant=v)  # noqa: E731
        err = float((fn(0).float() - ref).abs().max())
        t = timeit(fn)
        if v:
            best = min(best, t)
        else:
            t0 = t
        line += f" v{v} {t:6.1f} us ({gflop / t * 1e-3:4.0f} TF/s, err {err:.1e})" if v == 0 else f" v{v} {t:6.1f}"
    n = COUNT.get(name, 1)
    total["vendor"] += n * tv
    total["auto"] += n * t0
    total["best"] += n * best
    print(line, flush=True)
print("per frame (R50 layer counts):", {k: round(v, 1) for k, v in total.items()}, "us")
