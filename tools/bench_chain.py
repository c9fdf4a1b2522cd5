"""Standalone timing (hipGraph-captured) of the fused MLP-chain launches of the decoder, on each of the four kernels of
csrc/mlp_chain.hip. The kernels are chosen with the switches the tests use (routes.chain_rows4 / chain_transposed); the 32-row
kernel gets the launches without a sine stage at 8 x the row counts (a batch of 8 streams), which passes fused.WIDE_ROWS.
One line per (launch, kernel).
usage: python tools/bench_chain.py [library]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = {   # name -> (routes, batch)
    "r4": (dict(chain_rows4=True, chain_transposed=False), 1),
    "r32": (dict(chain_rows4=True, chain_transposed=False), 8),
    "r16": (dict(chain_rows4=False, chain_transposed=False), 1),
    "valu": (dict(chain_rows4=False, chain_transposed=True), 1),
}


def module_calls(batch=1):
    """[(name, rows, sine, fn)]: the five chain launches of a decoder layer at `batch` x their shipped row counts, seeded."""
    from simpb_amd.plugin.detection2d import SparseBox2DEncoder, SparseBox2DRefinementModule
    from simpb_amd.plugin.detection3d import SparseBox3DEncoder, SparseBox3DRefinementModule
    torch.manual_seed(0)
    enc3 = SparseBox3DEncoder([128, 32, 32, 64], vel_dims=3, mode="cat", output_fc=False, in_loops=1, out_loops=4).cuda().eval()
    enc2 = SparseBox2DEncoder(256, with_sin_embed=True, in_loops=1, out_loops=2).cuda().eval()
    r3 = SparseBox3DRefinementModule(256, num_cls=10, refine_yaw=True, with_quality_estimation=True).cuda().eval()
    r2 = SparseBox2DRefinementModule(256, num_cls=10, with_alpha_branch=True).cuda().eval()
    a3 = torch.randn(batch, 900, 11, device="cuda")
    f3, e3 = torch.randn(batch, 900, 256, device="cuda"), torch.randn(batch, 900, 256, device="cuda")
    a2 = torch.rand(batch, 1536, 2, device="cuda")
    f2, e2 = torch.randn(batch, 1536, 256, device="cuda"), torch.randn(batch, 1536, 256, device="cuda")
    dt = torch.full((batch,), 0.5, device="cuda")
    return [
        ("anchor encoder 3D (900 rows, 4 chains x 4 stages)", batch * 900, False, lambda: enc3(a3)),
        ("refine3d reg only (900)", batch * 900, False, lambda: r3(f3, a3, e3, time_interval=dt, return_cls=False)),
        ("refine3d reg+cls+quality (900)", batch * 900, False, lambda: r3(f3, a3, e3, time_interval=dt, return_cls=True)),
        ("encoder 2D sine (1536)", batch * 1536, True, lambda: enc2(a2)),
        ("refine2d reg+cls+alpha (1536)", batch * 1536, False, lambda: r2(f2, a2, e2)),
    ]


def timeit(fn, iters=30, reps=5):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(iters):
                fn()
        g.replay()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
    return a.elapsed_time(b) / (iters * reps) * 1e3


def main():
    if len(sys.argv) > 1:  # a variant library (experiments)
        import simpb_amd._lib as L
        L.LIB = os.path.abspath(sys.argv[1])
    from simpb_amd.plugin import fused, routes
    calls = {batch: module_calls(batch) for batch in sorted({b for _, b in KERNELS.values()})}
    for i, (name, _, _, _) in enumerate(calls[1]):
        for kernel, (route, batch) in KERNELS.items():
            _, rows, sine, fn = calls[batch][i]
            with routes.override(**route):
                want = {"r16": fused.R16, "valu": fused.VALU, "r4": fused.R4, "r32": fused.R32}[kernel]
                if fused.launch_form(rows, sine) != want:    # (the sine encoder never takes the 32-row kernel)
                    continue
                us = timeit(fn)
            print(f"{name:52s} {kernel:5s} {rows:6d} rows {us:8.1f} us", flush=True)


if __name__ == "__main__":
    main()
