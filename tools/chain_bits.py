"""Outputs of the four MLP-chain kernels (csrc/mlp_chain.hip) on fixed operands, one .npy of uint32 each, so that two builds
of the library can be compared bit for bit:

  python tools/chain_bits.py --lib OTHER/libsimpb_hip.so --out a && python tools/chain_bits.py --out b
  for every file: cmp a/<name>.npy b/<name>.npy

No timing and no tolerance; the operands are seeded and the kernels are deterministic (fixed summation order), so any
difference is a change in what the kernels compute. The launches, operands and kernel switches are those of
tests/test_mlp_chain_float64.py (imported, not copied). For every (kernel, launch) pair: every input kind of the launch at
N = 67 in both buffer layouts, the first kind at every row count of SWEEP, and for the m_live launches every `live` of that
test. Each item is the whole `out` buffer (sentinels included) plus every ln_out buffer. Then the five module calls of
tools/bench_chain.py at their shipped row counts under the default routes."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="load this build of the C-ABI library instead of the in-tree one")
    ap.add_argument("--out", required=True, help="directory for the .npy files")
    args = ap.parse_args()
    if args.lib:   # before first use, as bench.py --lib
        import simpb_amd._lib as _l
        _l.LIB = os.path.abspath(args.lib)
    import numpy as np
    import torch
    from tests import test_mlp_chain_float64 as T
    from tools import bench_chain

    os.makedirs(args.out, exist_ok=True)
    count = 0

    def save(name, t):
        nonlocal count
        a = t.detach().cpu().contiguous().numpy()
        assert a.dtype == np.float32, (name, a.dtype)
        np.save(os.path.join(args.out, name + ".npy"), a.view(np.uint32))
        count += 1

    def launch(name, kernel, launch_name, kind, n, layout, live=None):
        out, _, ln_bufs = T._run(kernel, launch_name, T._operands(launch_name, kind), n, layout, live=live)
        save(name + "_out", out)
        for j, buf in enumerate(ln_bufs):
            if buf is not None:
                save(f"{name}_ln{j}", buf)

    for kernel, launch_name in T._pairs():
        kinds = T._launches()[launch_name].kinds
        stem = f"{kernel}_{launch_name}"
        for layout in (0, 1):
            for kind in kinds:
                launch(f"{stem}_{kind}_n{T.N}_l{layout}", kernel, launch_name, kind, T.N, layout)
            for n in T.SWEEP:
                launch(f"{stem}_{kinds[0]}_n{n}_l{layout}", kernel, launch_name, kinds[0], n, layout)
        if launch_name in T._m_live_names(kernel):
            for i, live in enumerate(T._m_live_values(kernel)):
                launch(f"{stem}_{kinds[0]}_live{live}_l{i % 2}", kernel, launch_name, kinds[0], T.N, i % 2, live=live)

    with torch.no_grad():
        for i, (_, rows, _, fn) in enumerate(bench_chain.module_calls()):
            got = fn()
            for j, t in enumerate(got if isinstance(got, (tuple, list)) else [got]):
                if t is not None:
                    save(f"module{i}_rows{rows}_{j}", t)
    torch.cuda.synchronize()
    from simpb_amd import _lib
    print(f"chain_bits: {count} arrays in {args.out} from {_lib.LIB}")


if __name__ == "__main__":
    main()
