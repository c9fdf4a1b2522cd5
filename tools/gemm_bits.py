"""Outputs of the grouped GEMM kernels (csrc/gemm.hip) and of linear_split (csrc/linear_split.hip) on fixed operands,
one .npy each, so that two builds of the library can be compared bit for bit:

  python tools/gemm_bits.py --lib OTHER/libsimpb_hip.so --out a && python tools/gemm_bits.py --out b
  for every file: cmp a/<name>.npy b/<name>.npy

No timing and no tolerance; the operands are seeded and the kernels are deterministic (fixed summation order), so any
difference is a change in what the kernels compute. Operand sets: every shape of tests/test_split_range.py SHAPES and
of the test_gemm_vs_float64 table on both routes; rows outside the split window (the second pass); a grouped launch
with strided outputs and m_live; a wide-tile launch with m_live, the flagged second bias and the half-pair output;
both linear_split kernels with and without a row scaled by 2^20."""
import argparse
import math
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
    from simpb_amd.plugin import dense, routes
    from simpb_amd.plugin.ops import linear_split
    from tests import test_dense, test_split_range as sr

    os.makedirs(args.out, exist_ok=True)
    count = 0

    def save(name, t):
        nonlocal count
        a = t.detach().cpu().contiguous().numpy()
        np.save(os.path.join(args.out, name + ".npy"), a.view(np.uint32) if a.dtype == np.float32 else a)
        count += 1

    def both_routes(name, xs, w, b, relu):
        for route in (False, True):
            with routes.override(gemm_split_fp16=route):
                y = dense.linear([x.cuda() for x in xs], w.cuda(), b.cuda() if b is not None else None, relu=relu)
            save(f"{name}_{'split' if route else 'fp32'}", y)

    for name in sr.SHAPES:
        xs, w, b, relu = sr._operands(name)[:4]
        both_routes("range_" + name, xs, w, b, relu)
    for name in ("narrow32", "narrow64", "wide"):
        for case in ("x_outlier_1e6", "x_row_1e-9"):
            xs, w, _, relu = sr._operands(name)[:4]
            xs, w = sr._mixed(case, xs, w)
            both_routes(f"mixed_{name}_{case}", xs, w, None, relu)

    table = next(m.args[1] for m in test_dense.test_gemm_vs_float64.pytestmark if m.name == "parametrize" and m.args[0] == "m,n,ks,relu,bias")
    for m, n, ks, relu, bias in table:
        g = torch.Generator().manual_seed(m * 7 + n)
        xs = [torch.randn(m, k, generator=g) for k in ks]
        w = torch.randn(n, sum(ks), generator=g) / math.sqrt(sum(ks))
        b = torch.randn(n, generator=g) if bias else None
        both_routes(f"table_{m}x{n}_k{'_'.join(map(str, ks))}", xs, w, b, relu)

    # three jobs in one launch, strided input and output, m_live (tests/test_dense.py test_gemm_grouped_strided_and_m_live)
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(2, 50, 1536, generator=g).cuda()
    pos = torch.randn(2, 50, 256, generator=g).cuda()
    w0 = (torch.randn(512, 768, generator=g) / 28).cuda()
    w1 = (torch.randn(96, 256, generator=g) / 16).cuda()
    b1 = torch.randn(96, generator=g).cuda()
    big = torch.randn(1, 700, 128, generator=g).cuda()
    w2 = (torch.randn(64, 128, generator=g) / 11).cuda()
    live = torch.tensor([0, 0, 411], dtype=torch.int32, device="cuda")
    for route in (False, True):
        out1 = torch.full((2, 50, 200), 7.0, device="cuda")
        with routes.override(gemm_split_fp16=route):
            y0, _, y2 = dense.gemm(dense.job([wide[..., 512:1024], pos], w0),
                                   dense.job(pos, w1, b1, relu=True, out=out1[..., 100:196]),
                                   dense.job(big, w2, m_live=live[2:3]))
        for name, y in (("y0", y0), ("out1", out1), ("y2", y2)):
            save(f"grouped_{name}_{'split' if route else 'fp32'}", y)

    # the wide-tile form with m_live, row_flag / bias2 and the half-pair output
    g = torch.Generator().manual_seed(31)
    m, n, k, live_n = 3072, 1536, 512, 2260
    x = torch.randn(1, m, k, generator=g).cuda()
    w = (torch.randn(n, k, generator=g) / 22).cuda()
    b = torch.randn(n, generator=g).cuda()
    b2 = torch.randn(n, generator=g).cuda()
    flag = (torch.rand(m, generator=g) > 0.5).to(torch.int32).cuda()
    live = torch.tensor([live_n], dtype=torch.int32, device="cuda")
    save("wide_live_flag", dense.linear(x, w, b, m_live=live, row_flag=flag, bias2=b2))
    save("wide_live_flag_halfs", dense.linear(x, w, b, m_live=live, row_flag=flag, bias2=b2, split_halfs=True))

    # linear_split: f32 x (simpb_linear_f16x3) and f16 x (simpb_linear_f16in_split), plain and with one row * 2^20
    g = torch.Generator().manual_seed(300)
    x = torch.randn(300, 256, generator=g)
    w = (torch.randn(256, 256, generator=g) / 16).cuda()
    b = torch.randn(256, generator=g).cuda()
    big_row = x.clone()
    big_row[123] *= 2.0 ** 20
    for tag, xv in (("plain", x), ("row_2p20", big_row)):
        save(f"linear_f16x3_{tag}", linear_split(xv.cuda(), w, b))
        save(f"linear_f16in_{tag}", linear_split(xv.half().cuda(), w, b))
    torch.cuda.synchronize()
    from simpb_amd import _lib
    print(f"gemm_bits: {count} arrays in {args.out} from {_lib.LIB}")


if __name__ == "__main__":
    main()
