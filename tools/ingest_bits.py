"""Outputs of the ingest kernels (csrc/preprocess.hip, every instantiation) on fixed, seeded inputs, the f16 output and the u8
intermediate `mid` of every case as one .npy each, so that two builds of the library can be compared bit for bit:

  python tools/ingest_bits.py --lib OTHER/libsimpb_hip.so --out a && python tools/ingest_bits.py --out b
  for every file: cmp a/<name>.npy b/<name>.npy

No timing and no tolerance: the path is integer arithmetic and a table, so any differing byte is a change in what the kernels
compute. Inputs, layouts and rigs come from the ingest test modules and tests/planes_ref.py (imported, not copied); `mid` is
zeroed before each case, so the rows a skipped image leaves unwritten compare as well. Each case is the smallest shape at
which its path can still go wrong:
  F  every frame format at 30 x 50 (row bytes no multiple of 16) and 72 x 96, tight and in one padded layout, resize 0.5 (output
     widths 25 and 48). Tight bgr / nv12 / nv21 go through the two older entry points, with the host's vec16 off (50) and on (96);
  P  NV12 at pitch 100 (the alignment alternates from row to row), and BGR surfaces one byte past a 16-byte boundary;
  O  flip and to_rgb on and off (tight BGR, padded NV12);
  E  an enlargement and the one-tap identity (BGR, NV12);
  T  the contiguous batch and the address table of padded bgr, nv12 and p010;
  R  the five-camera rig of tests/test_gpu_rig_ingest.py, two streams, one address 0; the same at output width 38;
  A  roll: identity rows, 180, 3 and (on a square crop) 90 degrees, and the rolled rig of tests/test_gpu_roll.py with a null entry;
  X  full size, 1600 x 900 -> 704 x 256, six images, tight BGR and NV12."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(30, 50), (72, 96)]
HALF = dict(resize=0.5)
COLOUR = "bt601"      # (p010 takes no "jfif"; the RGB-order formats do not look at it)


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
    from simpb_amd import preprocess as P
    from tests import planes_ref as L
    from tests import test_gpu_plane_ingest as G, test_gpu_rig_ingest as RG, test_gpu_roll as RO, test_gpu_surface_ingest as SF
    from tests.test_gpu_preprocess import R50

    os.makedirs(args.out, exist_ok=True)
    count = 0

    def save(name, t, view):
        nonlocal count
        np.save(os.path.join(args.out, name.replace(" ", "_") + ".npy"), t.detach().cpu().contiguous().numpy().view(view))
        count += 1

    def case(name, plan, n, launch):
        """`launch()` of `n` images on `plan` with a zeroed intermediate: the output and `mid`."""
        plan.reserve(n, "cuda")
        plan.intermediate().zero_()
        out = launch()
        torch.cuda.synchronize()
        save(name + " out", out, np.uint16)
        save(name + " mid", plan.intermediate(), np.uint8)

    def tight(fmt, hw, n=2, seed=40):
        """Random tight frames as `pack` takes them (p010: the u16 samples, all 16 bits random)."""
        f = G.frames_of(fmt, hw, n, seed)
        return f.view(np.uint16) if fmt == "p010" else f

    def padded(fmt, hw):
        """One padded layout per format: a pitch that is no multiple of 16 (tests/test_gpu_plane_ingest.py for the newer ones)."""
        if fmt in L.NEW:
            return G.padded(fmt, hw)
        row = P.SurfaceLayout(hw, fmt).row_bytes
        return dict(pitch=row + 1) if fmt == "bgr" else dict(pitch=row + (2 if fmt == "p010" else 4), luma_rows=hw[0] + 2)

    def batch(plan, frames, fill=0xEE):
        """Tight frames as the contiguous device batch `plan.run` takes."""
        surf = L.pack(frames, plan.surface, fill)
        return torch.from_numpy(surf.reshape((-1,) + plan.frame_shape)).cuda()

    def run(name, plan, frames):
        dev = batch(plan, frames)
        case(name, plan, len(frames), lambda: plan.run(dev))

    def run_table(name, plan, frames, offset=0):
        held = G.own_allocations(L.pack(frames, plan.surface, 0xEE), offset)
        case(name, plan, len(held), lambda: plan.run_surfaces(held))

    # F: every format, tight and padded
    for fmt in P.FRAME_FORMATS:
        for hw in SIZES:
            for kind, kw in (("tight", None), ("padded", padded(fmt, hw))):
                run(f"F {fmt} {hw[0]}x{hw[1]} {kind}", P.ResamplePlan(hw, HALF, None, fmt, COLOUR, layout=kw), tight(fmt, hw))

    # P: pitch 100 and an off-boundary base
    frames, _ = SF.base_case()
    run("P nv12 pitch100", P.ResamplePlan((64, 96), HALF, None, "nv12", layout=dict(pitch=100)), frames)
    run_table("P bgr base+1", P.ResamplePlan((30, 50), HALF, layout=dict(pitch=160)), tight("bgr", (30, 50)), offset=1)

    # O: flip and to_rgb
    for flip in (False, True):
        for to_rgb in (False, True):
            aug, norm = dict(HALF, flip=flip), dict(P.IMG_NORM_CFG, to_rgb=to_rgb)
            run(f"O bgr tight flip{int(flip)} rgb{int(to_rgb)}", P.ResamplePlan((72, 96), aug, norm), tight("bgr", (72, 96)))
            run(f"O nv12 padded flip{int(flip)} rgb{int(to_rgb)}",
                P.ResamplePlan((30, 50), aug, norm, "nv12", layout=padded("nv12", (30, 50))), tight("nv12", (30, 50)))

    # E: an enlargement and the identity
    for fmt in ("bgr", "nv12"):
        run(f"E {fmt} enlarge", P.ResamplePlan((12, 20), dict(resize=2), None, fmt), tight(fmt, (12, 20)))
        plan = P.ResamplePlan((30, 50), dict(resize=1), None, fmt)
        assert plan.taps_x == plan.taps_y == 1
        run(f"E {fmt} identity", plan, tight(fmt, (30, 50)))

    # T: both forms of the images
    for fmt in ("bgr", "nv12", "p010"):
        for form, go in (("batch", run), ("table", run_table)):
            go(f"T {fmt} {form}", P.ResamplePlan((30, 50), HALF, None, fmt, COLOUR, layout=padded(fmt, (30, 50))), tight(fmt, (30, 50), 3, 41))

    # R: the rig
    for width in (40, 38):
        rig = P.RigPlan(RG.sources(width))
        tensors = RG.device_surfaces(1)
        tensors[3] = None
        case(f"R rig w{width} null3", rig, len(tensors), lambda: rig.run_surfaces(tensors))

    # A: roll
    dev = torch.from_numpy(RO.pictures(3, 7)).cuda()
    plan = P.ResamplePlan(RO.SRC, RO.AUG, roll=5)
    case("A identity rows", plan, 3, lambda: RO.run_rows(plan, dev, [P.ROLL_IDENTITY] * 3))
    for name, aug, roll in (("180", RO.AUG, 180), ("3", RO.AUG, 3), ("90 square", RO.SQUARE, 90)):
        plan = P.ResamplePlan(RO.SRC, aug, roll=roll)
        case(f"A roll {name}", plan, 3, lambda: plan.run(dev))
    sources, surfaces, _ = RO.rolled_rig()
    surfaces[1] = None
    rig = P.RigPlan(sources)
    case("A rig rolled null1", rig, len(surfaces), lambda: rig.run_surfaces(surfaces))

    # X: full size, the tight forms
    for fmt in ("bgr", "nv12"):
        run(f"X {fmt} r50", P.ResamplePlan((900, 1600), R50, None, fmt), tight(fmt, (900, 1600), 6, 42))

    print(f"ingest_bits: {count} arrays in {args.out} from {_lib.LIB}")


if __name__ == "__main__":
    main()
