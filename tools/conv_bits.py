"""Outputs of the backbone's convolution kernels (csrc/conv3x3.hip, csrc/conv1x1.hip) on fixed operands, one .npy each, so
that two builds of the library can be compared bit for bit:

  python tools/conv_bits.py --lib OTHER/libsimpb_hip.so --out a && python tools/conv_bits.py --out b
  for every file: cmp a/<name>.npy b/<name>.npy

No timing and no tolerance; the operands are seeded and the kernels are deterministic (fixed summation order), so any
difference is a change in what the kernels compute. The cases are the tables of the three test modules (imported, not
copied), kinds `randn` and `cancel`, ReLU off and on: 3x3 variants 1-8 over cases3; 9-11 and 12-13 over the maps, channel
counts and strides of their modules; variant 0 on SELECT3; the token forms (f32 + f16 and f16 alone) of variants 3, 7, 8,
12, 13 at TOK_MAP; the group launch on PYRAMID with every form mix of the resident module; conv1x1 variants 1-4 over
cases1 (plain, residual, 2x-upsampled residual, input_bias for variant 1, both strides)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("randn", "cancel")


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
    from simpb_amd.plugin.ops import conv1x1_nhwc, conv3x3_group_tokens, conv3x3_nhwc
    from tests import test_backbone_float64 as B, test_gpu_conv3x3_ksplit as KS, test_gpu_conv3x3_resident as RS

    os.makedirs(args.out, exist_ok=True)
    count = 0

    def save(name, t):
        nonlocal count
        a = t.detach().cpu().contiguous().numpy()
        np.save(os.path.join(args.out, name + ".npy"), a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint16))
        count += 1

    def tag(m, stride, cp, kind):
        return f"{'x'.join(map(str, m))}_s{stride}_{cp[0]}to{cp[1]}_{kind}"

    def maps3(name, variant, keys):
        for key in sorted(set(keys)):
            if key[3] not in KINDS:
                continue
            x, w, b = B.dev3(key)
            for relu in (False, True):
                save(f"{name}_{tag(*key)}_relu{int(relu)}", conv3x3_nhwc(x, w, b, relu=relu, stride=key[1], variant=variant))

    for v in range(1, 9):
        maps3(f"c3_v{v}", v, B.cases3(v))
    for v in sorted(KS.TILE):
        maps3(f"c3_v{v}", v, [(m, s, (cin, cout), k) for m in KS.maps_of(v) for cin in KS.CINS for cout in KS.COUTS for s in (1, 2) for k in KINDS])
    for v in sorted(RS.TH):
        maps3(f"c3_v{v}", v, [(m, 1, (cin, cout), k) for m in RS.maps_of(v) for cin in RS.CINS for cout in RS.COUTS for k in KINDS])
    maps3("c3_v0", 0, [(m, 1, cp, k) for m, cp, _ in B.SELECT3 for k in KINDS])

    # token rows: the buffers start as the sentinel, so a row that must stay untouched is part of the comparison
    per_cam, start = 3 * 5 + 9, 4
    for v in (3, 7, 8, 12, 13):
        for cp in ((64, 72), (128, 64)):
            for kind in KINDS:
                key = (B.TOK_MAP, 1, cp, kind)
                x, w, b = B.dev3(key)
                for f32 in (True, False):
                    t32, t16, _ = B.token_buffers(B.TOK_BS, B.TOK_CAMS * per_cam, cp[1], f32)
                    conv3x3_nhwc(x, w, b, relu=False, stride=1, tokens=(t32, per_cam, start, t16), variant=v)
                    name = f"tok_v{v}_{cp[0]}to{cp[1]}_{kind}_{'f32f16' if f32 else 'f16'}"
                    save(name + "_rows16", t16)
                    if f32:
                        save(name + "_rows32", t32)

    starts, at = [], 3
    for h, w in B.PYRAMID:
        starts.append(at)
        at += h * w + 2
    per_cam, n = at + 5, B.TOK_BS * B.TOK_CAMS
    for cp in ((256, 256), (64, 72)):
        for kind in KINDS:
            ds = [B.dev3(((n, h, w), 1, cp, kind)) for h, w in B.PYRAMID]
            for forms in ((8, 8, 8, 8), (13, 13, 13, 13), (13, 8, 13, 8), None):
                for f32 in (True, False):
                    t32, t16, _ = B.token_buffers(B.TOK_BS, B.TOK_CAMS * per_cam, cp[1], f32)
                    conv3x3_group_tokens([d[0] for d in ds], [d[1] for d in ds], [d[2] for d in ds], t32, per_cam, starts, col16=t16, variants=forms)
                    name = f"group_{'rule' if forms is None else '_'.join(map(str, forms))}_{cp[0]}to{cp[1]}_{kind}_{'f32f16' if f32 else 'f16'}"
                    save(name + "_rows16", t16)
                    if f32:
                        save(name + "_rows32", t32)

    for v in range(1, 5):
        for cin in B.CIN1:
            for key in B.cases1(cin):
                m, stride, _, cout, kind, form = key
                if kind not in KINDS or (form.startswith("inb") and v > 1):
                    continue
                x, w, b, res, inb = B.dev1(key)
                for relu in (False, True):
                    y = conv1x1_nhwc(x, w, b, residual=res, relu=relu, stride=stride, residual_upsample2x=form == "up", input_bias=inb, variant=v)
                    save(f"c1_v{v}_{tag(m, stride, (cin, cout), kind)}_{form}_relu{int(relu)}", y)
    torch.cuda.synchronize()
    from simpb_amd import _lib
    print(f"conv_bits: {count} arrays in {args.out} from {_lib.LIB}")


if __name__ == "__main__":
    main()
