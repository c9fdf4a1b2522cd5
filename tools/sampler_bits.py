"""Outputs of the deformable sampler kernels (csrc/deform_agg*.hip, dfa_prep.hip, msda*.hip, msda_prep of rowops.hip) on
fixed operands, one .npy each, so that two builds of the library can be compared bit for bit:

  python tools/sampler_bits.py --lib OTHER/libsimpb_hip.so --out a && python tools/sampler_bits.py --out b
  for every file: cmp a/<name>.npy b/<name>.npy

No timing and no tolerance; the operands are seeded and these outputs are deterministic (fixed summation order), so any
difference is a change in what the kernels compute. The cases are the tables of tests/test_samplers_float64.py and the
parameters of the two backward tests of tests/test_gpu_ops.py (imported, not copied):
  A  every A_CASES launch of the drop-in 3D operator (daf_fwd_rows / daf_fwd_generic);
  B  every B_CASES x token form and every B_MASKED x mask kind x token form of daf_fused_rows, with its loc_out and w_out;
     on the same operands dfa_points_kernel and dfa_weights_kernel (the three-launch route), unmasked and with each mask;
  C  every C_CASES x m_live x token form of msda_linear_fwd, and msda_prep_kernel on the same raw rows (with and without
     m_live);
  D  every D_CASES launch of msda_grouped_fwd;
  G  the backward operators on the cases of test_daf_backward_vs_autograd_of_oracle and
     test_msda_grouped_backward_vs_autograd_of_oracle: the gradients of the locations and of the weights / attention, which
     are plain stores in a fixed order. The gradients of the tokens / values are accumulated with float atomics in an order
     that differs from launch to launch; they are left out."""
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
    from simpb_amd import _lib
    from simpb_amd.plugin import ops
    from tests import test_gpu_ops as G, test_samplers_float64 as T

    os.makedirs(args.out, exist_ok=True)
    count = 0
    ptr, dev = ops._ptr, T.dev

    def save(name, t):
        nonlocal count
        a = t.detach().cpu().contiguous().numpy()
        np.save(os.path.join(args.out, name.replace(" ", "_") + ".npy"), a.view(np.uint32))
        count += 1

    for shape, bs, A, content in T.A_CASES:
        c = T.a_case(shape, bs, A, content)
        save(f"A {shape} bs{bs} A{A} {content}",
             ops.deformable_aggregation_function(dev(c["col"]), dev(c["ss"]), dev(c["st"]), dev(c["loc"]), dev(c["w"])))

    masks = dict(none=None, ones=np.ones((3, T.CAMS), np.uint8), drop=T.DROP)
    fused = [(f, l, "none") for f, l in T.B_CASES] + [(f, l, m) for f, l in T.B_MASKED for m in ("ones", "drop")]
    for family, logits, mask_kind in fused:
        c, mask = T.b_case(family, logits), masks[mask_kind]
        tokens, proj, cl = c["col"].copy(), c["proj"].copy(), c["cl"].copy()
        if mask is not None:      # as the test: nothing of a masked camera is read, so it holds NaN
            for b, cam in zip(*np.nonzero(mask == 0)):
                lo, hi = c["st"][cam, 0], c["st"][cam, -1] + c["ss"][cam, -1].prod()
                tokens[b, lo:hi], proj[b, cam], cl[b, cam] = np.nan, np.nan, np.nan
        anchor, learn, fix, wh, fl = (dev(c[k]) for k in ("anchor", "learn", "fix", "wh", "fl"))
        proj, cl, valid = dev(proj), dev(cl), dev(mask) if mask is not None else None
        name = f"B {family} {logits} {mask_kind}"
        for tok in ("f32", "f16"):
            feat = dev(tokens, torch.float16 if tok == "f16" else torch.float32).contiguous()
            out, loc, w = ops.dfa_fused(feat, dev(c["ss"]), dev(c["st"]), anchor, learn, fix, proj, wh, fl, cl, T.GRP,
                                        want_operands=True, cam_valid=valid)
            for part, t in (("out", out), ("loc", loc), ("w", w)):
                save(f"{name} {tok} {part}", t)
        if mask is None:
            save(f"{name} dfa_locations", ops.dfa_locations(anchor, learn, fix, proj, wh))
        bs, A = c["bs"], c["A"]
        loc3 = torch.empty(bs, A, T.NPTS, T.CAMS, 2, device="cuda")
        kp3 = torch.empty(bs, A, T.NPTS, 3, device="cuda")
        w3 = torch.empty(bs, A, T.NPTS, T.CAMS, T.LVL, T.GRP, device="cuda")
        vp = ptr(valid) if valid is not None else None
        _lib.check(_lib.lib().simpb_dfa_points_cams(ptr(loc3), ptr(kp3), ptr(anchor), ptr(learn), ptr(fix), ptr(proj), ptr(wh), bs, A,
                                                    T.NFIX, T.NLEARN, T.CAMS, vp, ops._stream()), "simpb_dfa_points_cams")
        _lib.check(_lib.lib().simpb_dfa_weights_cams(ptr(w3), ptr(fl), ptr(cl), bs, A, T.CAMS, T.LVL, T.NPTS, T.GRP, vp,
                                                     ops._stream()), "simpb_dfa_weights_cams")
        for part, t in (("points_loc", loc3), ("points_kp", kp3), ("weights", w3)):
            save(f"{name} three {part}", t)

    for bs, pyr in T.C_CASES:
        c = T.c_case(bs, pyr)
        ss, lsi = T.tables(c["shapes"])
        ss, lsi, raw, ref, qc = ss.cuda(), lsi.cuda(), dev(c["raw"]), dev(c["ref"]), dev(c["qc"])
        for use_m_live in (True, False):
            m_live = torch.tensor([T.M_LIVE], dtype=torch.int32, device="cuda") if use_m_live else None
            tag = f"C bs{bs} {pyr} {'m_live' if use_m_live else 'no_m_live'}"
            for tok in ("f16", "f32"):
                t = dev(c["tokens"], torch.float16 if tok == "f16" else torch.float32).contiguous()
                agg = ops.msda_linear(t, ss, lsi, raw, ref, qc, m_live)
                save(f"{tag} {tok}", agg[:, :T.M_LIVE if use_m_live else T.LIVE])      # the rows the launch owes
            rows, width = bs * T.NQ, raw.shape[-1]
            loc = torch.full((rows, T.S.HEADS, T.S.LVLS, T.S.PTS, 2), T.SENTINEL, device="cuda")
            attn = torch.full((rows, T.S.HEADS, T.S.LVLS, T.S.PTS), T.SENTINEL, device="cuda")
            _lib.check(_lib.lib().simpb_msda_prep(ptr(loc), ptr(attn), ptr(raw), width, ptr(ref), 2, ptr(ss), rows, T.S.HEADS, T.S.LVLS,
                                                  T.S.PTS, ptr(m_live) if use_m_live else None, ops._stream()), "simpb_msda_prep")
            save(f"{tag} prep loc", loc)
            save(f"{tag} prep attn", attn)

    for i, d in enumerate(T.D_CASES):
        c = T.d_case(i)
        ss, lsi = T.tables(c["shapes"])
        save(f"D pts{d['pts']} {d['heads'] * d['ch']}",
             ops.ms_deform_attn_grouped(dev(c["value"]), ss.cuda(), lsi.cuda(), dev(c["loc"]), dev(c["attn"]), dev(c["qc"])))

    R = G._oracle()
    (shapes,) = [m.args[1] for m in G.test_daf_backward_vs_autograd_of_oracle.pytestmark if m.name == "parametrize"]
    for n, s in enumerate(shapes):      # the operands of that test
        rs = np.random.RandomState(11)
        maps = [torch.from_numpy(rs.standard_normal((s["bs"], s["K"], s["C"], h, w)).astype(np.float32)) for h, w in s["maps"]]
        col, ss, ssi = R.feature_maps_format(maps)
        loc = torch.from_numpy(rs.uniform(-0.2, 1.2, (s["bs"], s["A"], s["P"], s["K"], 2)).astype(np.float32))
        w = torch.from_numpy(rs.uniform(0, 1, (s["bs"], s["A"], s["P"], s["K"], s["L"], s["G"])).astype(np.float32))
        gout = torch.from_numpy(rs.standard_normal((s["bs"], s["A"], s["C"])).astype(np.float32))
        c2, l2, w2 = (t.clone().cuda().requires_grad_() for t in (col, loc, w))
        ops.deformable_aggregation_function(c2, ss.int().cuda(), ssi.int().cuda(), l2, w2).backward(gout.cuda())
        save(f"G daf{n} grad_loc", l2.grad)
        save(f"G daf{n} grad_weights", w2.grad)
    cfg = dict(bs=2, nq=41, heads=8, ch=32, shapes=[(8, 22), (4, 11), (2, 6), (1, 3)], pts=4, ncam=6)   # (that test's one case)
    value, ss, lsi, loc, aw, groups = G._msda_inputs(seed=13, **cfg)
    gout = torch.from_numpy(np.random.RandomState(14).standard_normal((cfg["bs"], cfg["nq"], 256)).astype(np.float32))
    qcam = ops.query_cam_from_groups(groups, cfg["nq"], "cuda")
    v2, l2, a2 = (t.clone().cuda().requires_grad_() for t in (value, loc, aw))
    ops.ms_deform_attn_grouped(v2, ss.cuda(), lsi.cuda(), l2, a2, qcam).backward(gout.cuda())
    save("G msda grad_loc", l2.grad)
    save("G msda grad_attn", a2.grad)

    torch.cuda.synchronize()
    print(f"sampler_bits: {count} arrays in {args.out} from {_lib.LIB}")


if __name__ == "__main__":
    main()
