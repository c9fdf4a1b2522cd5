"""The per-launch table of profiles/image_skip.md, shared by tools/bench_stream_activity.py and tools/bench_camera_dropout.py:
three backbone launches of a bs 8 frame (48 images at 704 x 256) with all, half and one eighth of the images live, by device
events around a run of back-to-back launches. `full` is the launch without a table; the live sets are whole streams (six
consecutive images), the first ones, as a pause leaves them."""
import torch

IMAGES, PER_STREAM = 48, 6


def _time(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def launch_table(rounds=3):
    """[dict(launch, full_us, live_48_us, live_24_us, live_6_us)]: the median of `rounds` runs of 50 launches each."""
    import statistics
    from simpb_amd.plugin import ops
    from simpb_amd.runner import live_images
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)

    def rand(*shape, scale=0.5):
        return (torch.randn(*shape, generator=g) * scale).half().to(dev)

    def nchw(n, c, h, w):
        return rand(n, h, w, c).permute(0, 3, 1, 2)   # channels_last

    tables = {k: torch.from_numpy(live_images([s < k // PER_STREAM for s in range(IMAGES // PER_STREAM)], None,
                                              IMAGES // PER_STREAM, PER_STREAM)).to(dev) for k in (48, 24, 6)}
    x1, w1, b1 = nchw(IMAGES, 64, 64, 176), rand(64, 64, 3, 3, scale=0.04).contiguous(memory_format=torch.channels_last), rand(64)
    x3, w3, b3 = nchw(IMAGES, 256, 16, 44), rand(1024, 256, 1, 1, scale=0.04), rand(1024)
    r3 = nchw(IMAGES, 1024, 16, 44)
    shapes = ((64, 176), (32, 88), (16, 44), (8, 22))
    xs = [nchw(IMAGES, 256, h, w) for h, w in shapes]
    ws = [rand(256, 256, 3, 3, scale=0.02).contiguous(memory_format=torch.channels_last) for _ in shapes]
    bs_ = [rand(256) for _ in shapes]
    per_cam = sum(h * w for h, w in shapes)
    starts = [sum(h * w for h, w in shapes[:i]) for i in range(4)]
    col16 = torch.empty(IMAGES // PER_STREAM, PER_STREAM * per_cam, 256, device=dev, dtype=torch.float16)
    launches = {
        "layer1 conv2: 3x3, 64 -> 64, 64 x 176": lambda live: ops.conv3x3_nhwc(x1, w1, b1, live=live),
        "layer3 conv3: 1x1, 256 -> 1024 + residual, 16 x 44": lambda live: ops.conv1x1_nhwc(x3, w3, b3, r3, live=live),
        "FPN output convolutions, four levels in one launch (f16 rows)":
            lambda live: ops.conv3x3_group_tokens(xs, ws, bs_, None, per_cam, starts, col16, live=live),
    }
    rows = []
    for name, fn in launches.items():
        cols = dict(full=None, live_48=tables[48], live_24=tables[24], live_6=tables[6])
        got = {k: [] for k in cols}
        for _ in range(rounds):   # alternating: drift of the box hits every column alike
            for k, live in cols.items():
                got[k].append(_time(lambda: fn(live)))
        rows.append(dict(launch=name, **{k + "_us": round(statistics.median(v), 2) for k, v in got.items()}))
    return rows


def print_launch_table(rows):
    print("\nthe launches alone, 48 images, us per launch (median of alternating runs of 50)")
    print("| launch | no table | 48 live | 24 live | 6 live |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['launch']} | {r['full_us']} | {r['live_48_us']} | {r['live_24_us']} | {r['live_6_us']} |")
