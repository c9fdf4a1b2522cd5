"""Outputs of the attention kernels (csrc/attention.hip, all nine instantiations) on fixed operands, one .npy each, so that two
builds of the library can be compared bit for bit:

  python tools/attention_bits.py --lib OTHER/libsimpb_hip.so --out a && python tools/attention_bits.py --out b
  for every file: cmp a/<name>.npy b/<name>.npy

No timing and no tolerance; the operands are seeded and the kernels sum in a fixed order, so any difference is a change in
what they compute. Operands come from the _inputs of tests/test_attention_ungrouped.py and tests/test_attention_groups.py
(imported, not copied); split 2 runs on _pack_split_halfs operands with 1/8 folded into q, as the tests launch it.
  U  ungrouped, splits 0, 1, 2, inputs randn and sharp_ramp_up: nq = 65 at nk in U_NKS, and nq in U_NQS at nk = 45
     (attention_f32_kernel<false>, attention_f16s_kernel<false>, attention_halfs_kernel<false, 8>);
  G  grouped, splits 0, 1, 2, tables edges, no_group and r50_frame0, inputs randn and decay
     (attention_f32_kernel<true>, attention_f16s_kernel<true>, attention_halfs_kernel<true, 4>);
  S  the selector, splits 0, 1, 2, select (0, 1, 0) at the two SELECT_EDGES of the ungrouped module, the set a stream did
     not select poisoned with NaN (the three AltKeys instantiations)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U_NKS = [1, 32, 33, 128, 129, 255, 256, 257, 600, 900]
U_NQS = [1, 32, 33]
U_INPUTS = ["randn", "sharp_ramp_up"]
G_TABLES = ["edges", "no_group", "r50_frame0"]
G_INPUTS = ["randn", "decay"]


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
    from simpb_amd import _lib
    from simpb_amd.plugin.ops import attention_select
    from tests import test_attention_groups as G, test_attention_ungrouped as U
    from tests.test_gpu_stream_restart_ops import _poison

    os.makedirs(args.out, exist_ok=True)
    count = 0

    def save(name, t):
        nonlocal count
        a = t.detach().cpu().contiguous().numpy()
        np.save(os.path.join(args.out, name.replace(" ", "_") + ".npy"), a.view(np.uint32))
        count += 1

    for nq, nk in [(U.NQ, nk) for nk in U_NKS] + [(nq, 45) for nq in U_NQS]:
        for kind in U_INPUTS:
            q, k, v = U._inputs(nq, nk, kind)
            for split in U.SPLITS:
                save(f"U nq{nq} nk{nk} {kind} split{split}", U._launch(split, *(t.cuda() for t in U._as_launched(split, q, k, v))))

    for table in G_TABLES:
        bounds, n = G._table(table)
        tables = G._device_tables(bounds, n)
        for kind in G_INPUTS:
            q, k, v = G._inputs(table, kind)
            for split in (0, 1, 2):
                save(f"G {table} {kind} split{split}", G._run(q, k, v, split, tables))

    select = torch.tensor(U.SELECT, dtype=torch.uint8, device="cuda")
    for n1, n2 in U.SELECT_EDGES:
        q, sets = U._select_operands(n1, n2)
        for split in U.SPLITS:
            qd, k1, v1, k2, v2 = (t.clone() for t in U._as_launched(split, q, sets[0][0], sets[0][1], sets[1][0], sets[1][1]))
            for b, s in enumerate(U.SELECT):      # stream b never reads the set it did not select
                for t in ((k1, v1) if s else (k2, v2)):
                    _poison(t[b], split)
            save(f"S n{n1} n{n2} split{split}", attention_select(*(t.cuda() for t in (qd, k1, v1, k2, v2)), select, U.HEADS, split=split))

    torch.cuda.synchronize()
    print(f"attention_bits: {count} arrays in {args.out} from {_lib.LIB}")


if __name__ == "__main__":
    main()
