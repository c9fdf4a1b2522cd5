"""The four kernels behind simpb_mlp_chain_forward (csrc/mlp_chain.hip, host side plugin/fused.py) against float64, at the
row counts, widths, layouts and stages where each of them takes another path.

Kernels, chosen with the existing switches only (routes.chain_rows4 / chain_transposed, fused.WIDE_ROWS):
  r4    mlp_chain_r4_kernel (shipped): 4 rows per workgroup, k4-packed weights when K % 4 == 0, else one thread per column;
  r32   mlp_chain_r32_kernel (WIDE_ROWS = 1): 32 rows, fragment-packed weights when K % 32 == 0, else one thread per column;
  r16   mlp_chain_mfma_kernel: 16 rows, matrix path when K % 64 == 0, else one thread per column; 16-byte input loads when
        the width is a power of two and x, x2 and their row strides are 16-byte aligned;
  valu  mlp_chain_kernel<4, 8>: 4 rows, split-K with 16-byte weight loads when D % 4 == 0 and K >= 16, else per column.
The host keeps sine chains on the 4-row kernel, so (r32, sine) does not exist; a leading LayerNorm exists in r4 and r32 only.

Reference: tests/chain_ref.py in float64; its float32 evaluation is the "plain fp32" baseline. Bounds, the project's own:
  (a) every output finite wherever float64 is;
  (b) max |got - want| <= 2e-5 * max(1, max |want|) on randn, big, zero_rows, the sine points and the post-stage edges
      (bound (b) of tests/test_attention_groups.py); test_fp32_formula_stays_under_half_of_bound_b holds plain fp32 to half
      of it on every (launch, input, row count) that the GPU tests apply it to;
  (c) on offset and const rows fp32 itself loses digits in a LayerNorm (the mean's rounding error is divided by a deviation
      of 1e-2, or by sqrt(eps)), so there max |got - want| <= 4 * e32 + 1e-7 * max(1, max |want|) per output tensor, e32 the
      error of the float32 evaluation of chain_ref on the same operands (second line of tests/test_split_range._check);
  (d) a row's output bits do not depend on its position or on the other rows (torch.equal), on launches without `div`.
Every output buffer is filled with a sentinel first: columns between the chains' ranges, the pad behind them and rows past
num_rows must still hold it. Input buffers hold NaN wherever no operand lies. Measured figures of one MI355X run:
profiles/mlp_chain_vs_float64.md.

Inputs, N = 67 rows seeded per (launch, input); a smaller row count takes the first rows of the same operands:
  randn      N(0, 1);
  big        N(0, 1) * 1e3;
  zero_rows  randn with x and x2 zero on rows 0, 4-7 (a whole 4-row tile), 33 and 66: behind a Linear without bias ReLU
             leaves a constant row, whose LayerNorm goes through eps;
  offset     rows of mean 30 and deviation 1e-2;
  const      row i holds the single value 10 * c_i, c_i ~ N(0, 1);
  points     sine chains: (x, y) uniform in [-0.5, 1.5]^2, and the exact corners (0, 0), (1, 1), (0, 1), (1, 0).
Post-stage operands are the same for every input: REFINE2D residuals uniform in [0, 1] with rows of (0, 1), (1e-6, 1 - 1e-6)
and (-0.2, 1.2); REFINE3D residuals N(0, 1) and div = (0.5, 0.37) over two batches of 34 rows (no tile size divides 34);
the `sig` and `post2d` heads carry biases of +-100 into their sigmoids, and `post2d` biases of +6 / -6 on its two residual
columns, so that the clamped ends of inverse_sigmoid (-+11.5) land where the sigmoid still moves."""
import contextlib
import copy
import math

import pytest
import torch
import torch.nn as nn

from simpb_amd import synth
from tests.chain_ref import POST_REFINE2D, POST_REFINE3D, POST_SIGMOID, chain_ref

gpu = pytest.mark.gpu
N = 67
SENT = -12345.0
SWEEP = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33]      # one less / equal / one more than each row tile (4, 16, 32), and one row
ZERO_ROWS = [0, 4, 5, 6, 7, 33, 66]
DIV_ROWS = 34
KERNELS = {   # switches and the row tile
    "r4": dict(rows4=True, transposed=False, wide=False, R=4),
    "r32": dict(rows4=True, transposed=False, wide=True, R=32),
    "r16": dict(rows4=False, transposed=False, wide=False, R=16),
    "valu": dict(rows4=False, transposed=True, wide=False, R=4),
}


# ---------------------------------------------------------------------------------------------------- programs
def L(k, d, relu=True):
    return ("L", k, d, relu)


def LN(d):
    return ("N", d)


def _program(spec, seed, scale=False, first_bias=True, last_bias=()):
    """nn.Sequential of `spec` with seeded weights of ordinary scale: W ~ N(0, 1) / sqrt(K), b ~ 0.1 N(0, 1), LayerNorm gains
    1 + 0.2 N(0, 1) and biases 0.1 N(0, 1), Scale 1 + 0.3 N(0, 1). last_bias: (column, value) pairs set on the last Linear."""
    from simpb_amd.plugin.layers import Scale
    g = torch.Generator().manual_seed(seed)
    mods, last = [], None
    with torch.no_grad():
        for i, op in enumerate(spec):
            if op[0] == "L":
                _, k, d, relu = op
                last = nn.Linear(k, d, bias=first_bias or i > 0)
                last.weight.copy_(torch.randn(d, k, generator=g) / math.sqrt(k))
                if last.bias is not None:
                    last.bias.copy_(0.1 * torch.randn(d, generator=g))
                mods.append(last)
                if relu:
                    mods.append(nn.ReLU())
            else:
                ln = nn.LayerNorm(op[1])
                ln.weight.copy_(1 + 0.2 * torch.randn(op[1], generator=g))
                ln.bias.copy_(0.1 * torch.randn(op[1], generator=g))
                mods.append(ln)
        for col, value in last_bias:
            last.bias[col] = value
        if scale:
            mods.append(Scale((1 + 0.3 * torch.randn(last.out_features, generator=g)).tolist()))
    return nn.Sequential(*mods)


def _norm(width, seed):
    g = torch.Generator().manual_seed(seed)
    ln = nn.LayerNorm(width)
    with torch.no_grad():
        ln.weight.copy_(1 + 0.2 * torch.randn(width, generator=g))
        ln.bias.copy_(0.1 * torch.randn(width, generator=g))
    return ln


class Job:
    """One chain of a launch. post: dict(kind, res_cols, div_col0 or None)."""

    def __init__(self, seq, x2=False, sine=False, ln=None, ln_out=False, post=None):
        lins = [m for m in seq if isinstance(m, nn.Linear)]
        first = next(m for m in seq if isinstance(m, (nn.Linear, nn.LayerNorm)))
        self.seq, self.x2, self.sine, self.ln, self.ln_out, self.post = seq, x2, sine, ln, ln_out, post
        self.in_dim = first.in_features if isinstance(first, nn.Linear) else first.normalized_shape[0]
        self.out_dim = lins[-1].out_features if lins else self.in_dim
        self.in_cols = 2 if sine else self.in_dim


class Launch:
    def __init__(self, name, jobs):
        self.name, self.jobs, self._cuda = name, jobs, None
        self.sine = any(j.sine for j in jobs)
        self.lead_ln = any(j.ln is not None for j in jobs)
        self.kinds = ["points"] if self.sine else ["randn", "big", "zero_rows"]

    def kernels(self):
        return [k for k in KERNELS if not (k == "r32" and self.sine) and not (self.lead_ln and k in ("r16", "valu"))]

    def cuda(self):
        """[(seq, leading norm)] on the device; the plans (and their repacked weights) live on these copies."""
        if self._cuda is None:
            self._cuda = [(copy.deepcopy(j.seq).cuda(), copy.deepcopy(j.ln).cuda() if j.ln is not None else None)
                          for j in self.jobs]
        return self._cuda


def _width_specs():
    return {
        # K = 3: one thread per column in all four kernels (3 % 4, 3 % 32, 3 % 64, 3 < 16); K = 128 = 32 packed steps (r4),
        # four fragment chunks (r32), two 64-chunks (r16), 16 k per wave (valu)
        "w1": [L(3, 128), LN(128), L(128, 128), LN(128)],
        # K = 12: packed in r4 (12 % 4 == 0), per column in r32 (12 % 32), r16 (12 % 64) and valu (12 < 16);
        # K = 32: ONE fragment chunk in r32 (the clamped prefetch re-requests it), per column in r16 (32 % 64), wide in valu
        "w2": [L(12, 32), LN(32), L(32, 32), LN(32)],
        # D = 100: partial 32-column (r32) and 64-column (r4, r16) tile; K = 100: 25 packed steps = 3 full groups + 1 (r4), a
        # ragged 8-way split 13 x 7 + 9 (valu), nn.Linear's layout in r32 (100 % 32) and r16 (100 % 64); D = 65: one column
        # past a tile, per column in valu (65 % 4); K = 65: odd, per column everywhere; LayerNorm widths 100 and 65 leave
        # masked lanes in the reductions; D = 7: one partly filled tile
        "w3": [L(64, 100), LN(100), L(100, 65), LN(65), L(65, 7, False)],
        # K = 256: the full four 64-chunks (r16), eight fragment chunks (r32), 64 packed steps (r4); two Linears back to back;
        # D = 255: last column of the last tile missing, per column in valu (255 % 4); K = 255: per column everywhere;
        # LayerNorm width 255: one masked lane; D = 1
        "w4": [L(256, 256), L(256, 256), LN(256), L(256, 255), LN(255), L(255, 1, False)],
        # K = 192: three 64-chunks with the clamped prefetch (r16), six fragment chunks (r32); K = 96: three chunks in r32 (the
        # last `work` of a pair is skipped), 24 packed steps = an odd group count in r4, per column in r16 (96 % 64);
        # K = 160: five chunks in r32, per column in r16; D = 160: five column tiles, one wave owns a lone tile (r32), a
        # Linear without ReLU in front of a LayerNorm; D = 33: a second tile of one column
        "w5": [L(192, 96), LN(96), L(96, 160, False), LN(160), L(160, 33, False)],
        # SIMPB_MLP_MAX_OPS = 12 ops; K = 16 and K = 20: the first widths of valu's wide path (K >= 16), K = 20 = 5 packed steps
        "ops12": [L(16, 48), LN(48), L(48, 20), LN(20), L(20, 64), LN(64), L(64, 36, False), LN(36), L(36, 36), LN(36),
                  L(36, 5), L(5, 9, False)],
        # a program that starts with a LayerNorm op (width 100: masked lanes), for the ill-conditioned rows
        "lnfirst": [LN(100), L(100, 64), LN(64), L(64, 10, False)],
    }


_LAUNCHES = {}


def _launches():
    if _LAUNCHES:
        return _LAUNCHES
    from simpb_amd.plugin.detection2d import SparseBox2DEncoder, SparseBox2DRefinementModule
    from simpb_amd.plugin.detection3d import SparseBox3DEncoder, SparseBox3DRefinementModule
    enc = SparseBox3DEncoder(embed_dims=[128, 32, 32, 64], vel_dims=3, mode="cat", output_fc=False, in_loops=1, out_loops=4)
    enc2 = SparseBox2DEncoder(embed_dims=256, with_sin_embed=True, in_loops=1, out_loops=2)
    ref3 = SparseBox3DRefinementModule(embed_dims=256, num_cls=10, refine_yaw=True, with_quality_estimation=True)
    ref2 = SparseBox2DRefinementModule(embed_dims=256, num_cls=10, with_alpha_branch=True)
    for seed, m in enumerate((enc, enc2, ref3, ref2)):
        synth.load_procedural(m, seed=31 + seed)
    post3 = dict(kind=POST_REFINE3D, res_cols=11, div_col0=8)
    post2 = dict(kind=POST_REFINE2D, res_cols=2, div_col0=None)

    def add(name, jobs):
        _LAUNCHES[name] = Launch(name, jobs)

    # ---- shipped programs
    add("enc3d", [Job(enc.pos_fc), Job(enc.size_fc), Job(enc.yaw_fc), Job(enc.vel_fc)])   # four branches, one output
    add("enc2d_sine", [Job(enc2.query_embeddings2d, sine=True)])
    add("ref3d", [Job(ref3.layers, x2=True, post=post3), Job(ref3.cls_layers), Job(ref3.quality_layers, x2=True)])
    add("ref2d", [Job(ref2.layers, x2=True, post=post2), Job(ref2.cls_layers), Job(ref2.alpha_layers)])
    n3, n2 = _norm(256, 41), _norm(256, 42)
    add("ref3d_norm", [Job(ref3.layers, x2=True, post=post3, ln=n3, ln_out=True), Job(ref3.cls_layers, ln=n3),
                       Job(ref3.quality_layers, x2=True, ln=n3)])
    add("ref2d_norm", [Job(ref2.layers, x2=True, post=post2, ln=n2, ln_out=True), Job(ref2.cls_layers, ln=n2),
                       Job(ref2.alpha_layers, ln=n2)])
    # ---- width programs
    specs = _width_specs()
    w = {
        "w1": _program(specs["w1"], 51),
        "w2": _program(specs["w2"], 52, first_bias=False),     # Linear without bias
        "w3": _program(specs["w3"], 53, scale=True),
        "w4": _program(specs["w4"], 54, first_bias=False),
        "w5": _program(specs["w5"], 55),
        "ops12": _program(specs["ops12"], 56),
        "lnfirst": _program(specs["lnfirst"], 57),
    }
    add("w1", [Job(w["w1"])])
    add("w2", [Job(w["w2"])])
    add("w3", [Job(w["w3"], x2=True)])
    add("w4", [Job(w["w4"])])
    add("w5", [Job(w["w5"], x2=True)])
    add("ops12", [Job(w["ops12"])])
    add("lnfirst", [Job(w["lnfirst"])])
    # leading LayerNorm of a width that leaves masked lanes, in front of the tail of w3
    tail = _program(specs["w3"][2:], 58, scale=True)
    add("lnlead100", [Job(tail, x2=True, ln=_norm(100, 43), ln_out=True)])
    # post-stage heads with logits of +-100 in front of the sigmoids
    sig = _program([L(32, 32), LN(32), L(32, 6, False)], 59, scale=True, last_bias=((0, 100.0), (1, -100.0)))
    # (post2d: +-6 on the residual columns too: the clamped ends of inverse_sigmoid are logits of -+11.5, which alone
    # saturate the sigmoid and would hide a wrong clamp from an absolute bound; residual rows hold (low, high) pairs)
    p2d = _program([L(64, 64), LN(64), L(64, 4, False)], 60, scale=True,
                   last_bias=((0, 6.0), (1, -6.0), (2, 100.0), (3, -100.0)))
    add("sig", [Job(sig, post=dict(kind=POST_SIGMOID, res_cols=0, div_col0=None))])
    add("post2d", [Job(p2d, x2=True, post=post2)])
    # SIMPB_MLP_MAX_CHAINS = 8 chains with different programs, widths, row strides and column offsets
    add("chains8", [Job(w["w1"]), Job(w["w2"]), Job(w["w3"], x2=True), Job(w["w5"]), Job(w["ops12"], x2=True),
                    Job(sig, post=dict(kind=POST_SIGMOID, res_cols=0, div_col0=None)), Job(p2d, post=post2),
                    Job(enc.yaw_fc)])
    return _LAUNCHES


NAMES = ["enc3d", "enc2d_sine", "ref3d", "ref2d", "ref3d_norm", "ref2d_norm", "w1", "w2", "w3", "w4", "w5", "ops12", "lnfirst",
         "lnlead100", "sig", "post2d", "chains8"]
ALL_KINDS = ["randn", "big", "zero_rows", "offset", "const", "points"]


def _pairs(names=NAMES):
    """(kernel, launch name) for every pair that exists; built from the names so that collection imports nothing heavy."""
    out = []
    for name in names:
        for k in KERNELS:
            if (k == "r32" and name.endswith("_sine")) or (k in ("r16", "valu") and ("norm" in name or "lnlead" in name)):
                continue
            out.append((k, name))
    return out


# ---------------------------------------------------------------------------------------------------- operands, reference
_OPS, _REF = {}, {}


def _operands(name, kind):
    """Per job dict(x, x2, post) on N rows, CPU float32; post in chain_ref's form."""
    if (name, kind) in _OPS:
        return _OPS[name, kind]
    launch = _launches()[name]
    g = torch.Generator().manual_seed(1000 * NAMES.index(name) + ALL_KINDS.index(kind) + 1)
    ops = []
    for job in launch.jobs:
        w = job.in_cols
        x = torch.randn(N, w, generator=g)
        x2 = torch.randn(N, w, generator=g) if job.x2 else None
        if job.sine:
            x = torch.rand(N, 2, generator=g) * 2 - 0.5
            x[:4] = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]])
        elif kind == "big":
            x, x2 = x * 1e3, (x2 * 1e3 if job.x2 else None)
        elif kind == "zero_rows":
            x[ZERO_ROWS] = 0
            if job.x2:
                x2[ZERO_ROWS] = 0
        elif kind == "offset":
            x = 30 + 1e-2 * x
        elif kind == "const":
            x = (10 * torch.randn(N, 1, generator=g)).expand(N, w).contiguous()
        post = None
        if job.post is not None:
            post = dict(kind=job.post["kind"], res_cols=job.post["res_cols"], res=None, div=None, div_rows=DIV_ROWS,
                        div_col0=job.post["div_col0"])
            if job.post["kind"] == POST_REFINE2D:
                res = torch.rand(N, 2, generator=g)
                res[:3] = torch.tensor([[0.0, 1.0], [1e-6, 1 - 1e-6], [-0.2, 1.2]])
                post["res"] = res
            elif job.post["kind"] == POST_REFINE3D:
                post["res"] = torch.randn(N, 11, generator=g)
                post["div"] = torch.tensor([0.5, 0.37])
        ops.append(dict(x=x, x2=x2, post=post))
    _OPS[name, kind] = ops
    return ops


def _reference(name, kind):
    """Per job (want, ln_want, fp32, ln_fp32): chain_ref in float64 and in float32 on the N rows, computed once."""
    if (name, kind) not in _REF:
        launch = _launches()[name]
        refs = []
        for job, op in zip(launch.jobs, _operands(name, kind)):
            with torch.no_grad():
                a = chain_ref(job.seq, op["x"], op["x2"], sine=job.sine, ln=job.ln, post=op["post"])
                b = chain_ref(job.seq, op["x"], op["x2"], sine=job.sine, ln=job.ln, post=op["post"], dtype=torch.float32)
            refs.append((a[0], a[1] if job.ln_out else None, b[0], b[1] if job.ln_out else None))
        _REF[name, kind] = refs
    return _REF[name, kind]


def _ratio_b(got, want):
    if not want.numel():
        return 0.0
    return float((got.double() - want).abs().max()) / (2e-5 * max(1.0, float(want.abs().max())))


def _ratio_c(got, want, fp32):
    e32 = float((fp32.double() - want).abs().max())
    return float((got.double() - want).abs().max()) / (4 * e32 + 1e-7 * max(1.0, float(want.abs().max())))


def _b_cases():
    """(launch name, input, row count) of every application of bound (b) in the GPU tests."""
    for name in NAMES:
        for kind in _launches()[name].kinds:
            yield name, kind, N
        for n in SWEEP:   # also the row prefixes that the m_live test holds to (b)
            yield name, _launches()[name].kinds[0], n


# ---------------------------------------------------------------------------------------------------- CPU
def test_chain_ref_float64_equals_the_shipped_modules_in_double():
    """chain_ref in float64 against the modules themselves after .double() on the CPU, to 1e-12: the anchor encoder's four
    branches, the sine encoder (pos2posemb2d), both refinement heads with their post formulas, with the clamped ends of
    inverse_sigmoid and two time intervals."""
    from simpb_amd.plugin.detection2d import SparseBox2DEncoder, SparseBox2DRefinementModule
    from simpb_amd.plugin.detection3d import SparseBox3DEncoder, SparseBox3DRefinementModule
    g = torch.Generator().manual_seed(5)
    enc = SparseBox3DEncoder(embed_dims=[128, 32, 32, 64], vel_dims=3, mode="cat", output_fc=False, in_loops=1, out_loops=4)
    enc2 = SparseBox2DEncoder(embed_dims=256, with_sin_embed=True, in_loops=1, out_loops=2)
    ref3 = SparseBox3DRefinementModule(embed_dims=256, num_cls=10, refine_yaw=True, with_quality_estimation=True)
    ref2 = SparseBox2DRefinementModule(embed_dims=256, num_cls=10, with_alpha_branch=True)
    for seed, m in enumerate((enc, enc2, ref3, ref2)):
        synth.load_procedural(m, seed=21 + seed)
        m.double()
    n = 2 * DIV_ROWS
    box = torch.randn(n, 11, generator=g)
    pts = torch.rand(n, 2, generator=g) * 2 - 0.5
    pts[:2] = torch.tensor([[0.0, 1.0], [1.0, 0.0]])
    f, e = torch.randn(n, 256, generator=g), torch.randn(n, 256, generator=g)
    a2 = torch.rand(n, 2, generator=g)
    a2[:3] = torch.tensor([[0.0, 1.0], [1e-6, 1 - 1e-6], [-0.2, 1.2]])
    dt = torch.tensor([0.5, 0.37])
    pairs = []
    with torch.no_grad():
        want = enc(box.double())
        got = torch.cat([chain_ref(s, box[:, a:b])[0] for s, (a, b) in
                         ((enc.pos_fc, (0, 3)), (enc.size_fc, (3, 6)), (enc.yaw_fc, (6, 8)), (enc.vel_fc, (8, 11)))], -1)
        pairs.append(("enc3d", got, want))
        pairs.append(("enc2d_sine", chain_ref(enc2.query_embeddings2d, pts, sine=True)[0], enc2(pts.double())))
        w_out, w_cls, w_q = ref3(f.double().reshape(2, DIV_ROWS, 256), box.double().reshape(2, DIV_ROWS, 11),
                                 e.double().reshape(2, DIV_ROWS, 256), dt.double(), True)
        post3 = dict(kind=POST_REFINE3D, res=box, res_cols=11, div=dt, div_rows=DIV_ROWS, div_col0=8)
        pairs.append(("ref3d box", chain_ref(ref3.layers, f, e, post=post3)[0], w_out.reshape(n, 11)))
        pairs.append(("ref3d cls", chain_ref(ref3.cls_layers, f)[0], w_cls.reshape(n, 10)))
        pairs.append(("ref3d quality", chain_ref(ref3.quality_layers, f, e)[0], w_q.reshape(n, 2)))
        w_box, w_cls, _, w_al = ref2(f.double(), a2.double(), e.double())
        post2 = dict(kind=POST_REFINE2D, res=a2, res_cols=2)
        pairs.append(("ref2d box", chain_ref(ref2.layers, f, e, post=post2)[0], w_box))
        pairs.append(("ref2d cls", chain_ref(ref2.cls_layers, f)[0], w_cls))
        pairs.append(("ref2d alpha", chain_ref(ref2.alpha_layers, f)[0], w_al))
        ln = _norm(256, 1).double()
        got, ln_out = chain_ref(ref2.cls_layers, f, e, ln=ln)
        pairs.append(("leading norm", got, ref2.cls_layers(ln(f.double()) + e.double())))
        pairs.append(("ln_out", ln_out, ln(f.double())))
        pairs.append(("sigmoid", chain_ref(ref2.cls_layers, f, post=dict(kind=POST_SIGMOID))[0], w_cls.sigmoid()))
    for what, got, want in pairs:
        assert got.dtype == torch.float64 and got.shape == want.shape, what
        assert float((got - want).abs().max()) <= 1e-12, (what, float((got - want).abs().max()))


def test_fp32_formula_stays_under_half_of_bound_b():
    """The float32 evaluation of chain_ref stays under HALF of (b) on every (launch, input, row count) that the GPU tests
    apply (b) to, ln_out included: a correct fp32-grade kernel can meet the bound."""
    over = []
    worst = {}
    for name, kind, n in _b_cases():
        for j, (want, ln_want, fp32, ln_fp32) in enumerate(_reference(name, kind)):
            r = _ratio_b(fp32[:n], want[:n])
            if ln_want is not None:
                r = max(r, _ratio_b(ln_fp32[:n], ln_want[:n]))
            worst[name, kind] = max(worst.get((name, kind), 0.0), r)
            if r > 0.5:
                over.append((name, kind, n, j, r))
    for (name, kind), r in worst.items():
        print("FP32|%s|%s|b=%.3f" % (name, kind, r))
    assert not over, over


def test_launch_table_fits_the_kernel_limits():
    from simpb_amd.plugin import fused
    launches = _launches()
    assert sorted(launches) == sorted(NAMES)
    assert len(launches["chains8"].jobs) == fused.MAX_CHAINS
    assert len(fused.ChainPlan(launches["ops12"].jobs[0].seq).ops) == fused.MAX_OPS
    for k, name in _pairs():
        assert k in launches[name].kernels()
    assert len(_pairs()) == sum(len(launch.kernels()) for launch in launches.values())


def test_leading_layernorm_is_refused_by_the_16_row_and_valu_routes():
    """A leading LayerNorm exists in the 4-row and 32-row kernels only: run_chains raises before anything is launched."""
    from simpb_amd.plugin import fused, routes
    job = _launches()["lnlead100"].jobs[0]
    x, out = torch.zeros(4, 100), torch.zeros(4, 7)
    for rows4, transposed in ((False, False), (False, True)):
        with routes.override(chain_rows4=rows4, chain_transposed=transposed):
            with pytest.raises(ValueError):
                fused.run_chains([dict(plan=fused.ChainPlan(job.seq), x=(x, 100, 0), out=(out, 7, 0), ln=(job.ln, None))],
                                 4, x.device)


# ---------------------------------------------------------------------------------------------------- GPU
@contextlib.contextmanager
def _kernel(name):
    from simpb_amd.plugin import fused, routes
    k = KERNELS[name]
    keep = fused.WIDE_ROWS
    try:
        fused.WIDE_ROWS = 1 if k["wide"] else 1 << 30
        with routes.override(chain_rows4=k["rows4"], chain_transposed=k["transposed"]):
            yield
    finally:
        fused.WIDE_ROWS = keep


def _place(t, col, layout, rows=None, fill=float("nan")):
    """t [n, w] at column `col` of a device buffer with a row stride larger than col + w: (buffer, stride, col).
    layout 0: col and stride multiples of 4 (16-byte aligned rows); layout 1: a stride that is no multiple of 4."""
    n, w = t.shape
    ld = (col + w + 3) // 4 * 4 + 4 if layout == 0 else col + w + 2
    if layout == 1 and ld % 4 == 0:
        ld += 1
    buf = torch.full((rows or n, ld), fill, dtype=torch.float32)
    buf[:n, col:col + w] = t
    return buf.cuda(), ld, col


def _run(kernel, name, ops, n, layout, live=None):
    """One launch of `name` on the first n rows of `ops`. Returns (out [n + 2, ldo], column span per job, ln_out buffers
    [n + 2, ld] or None per job), on the CPU. layout 0: x at column 4, x2 at column 8, outputs 4 columns apart; layout 1: x
    at column 3 (off the 16-byte input path of the 16-row kernel), x2 at column 1, outputs 1 or 3 columns apart."""
    from simpb_amd.plugin import fused
    launch = _launches()[name]
    gaps = (4, 4) if layout == 0 else (1, 3)
    spans, col = [], 0
    for j, job in enumerate(launch.jobs):
        col += gaps[j % 2]
        spans.append((col, col + job.out_dim))
        col += job.out_dim
    ldo = col + gaps[0]
    out = torch.full((n + 2, ldo), SENT, dtype=torch.float32, device="cuda")
    jobs, ln_bufs = [], []
    for j, (job, op, (seq, ln)) in enumerate(zip(launch.jobs, ops, launch.cuda())):
        d = dict(plan=fused.plan_of(seq), x=_place(op["x"][:n], 4 if layout == 0 else 3, layout), out=(out, ldo, spans[j][0]),
                 sine=job.sine)
        if op["x2"] is not None:
            d["x2"] = _place(op["x2"][:n], 8 if layout == 0 else 1, layout)
        ln_buf = None
        if ln is not None:
            if job.ln_out:
                ln_buf = _place(torch.empty(0, job.in_dim), 0, layout, rows=n + 2, fill=SENT)
            d["ln"] = (ln, ln_buf[:2] if ln_buf is not None else None)
        ln_bufs.append(ln_buf)
        if op["post"] is not None:
            p = op["post"]
            d["post"] = dict(kind=p["kind"], res_cols=p["res_cols"])
            if p["res"] is not None:
                d["post"]["res"] = _place(p["res"][:n], 0, layout)[:2]
            if p["div"] is not None:
                d["post"].update(div=p["div"].cuda(), div_rows=p["div_rows"], div_col0=p["div_col0"])
        jobs.append(d)
    ml = torch.tensor([live], dtype=torch.int32, device="cuda") if live is not None else None
    with _kernel(kernel):
        fused.run_chains(jobs, n, out.device, m_live=ml)
    torch.cuda.synchronize()
    return out.cpu(), spans, [b[0].cpu() if b is not None else None for b in ln_bufs]


def _assert_unowned(out, spans, n, what):
    """Columns between and behind the chains' ranges and rows past num_rows still hold the sentinel."""
    free = torch.ones_like(out, dtype=torch.bool)
    for a, b in spans:
        free[:n, a:b] = False
    assert bool((out[free] == SENT).all()), (what, "a column or row that no chain owns was written")


def _assert_ln_unowned(buf, width, n, what):
    assert bool((buf[:, width:] == SENT).all()) and bool((buf[n:] == SENT).all()), (what, "ln_out written outside its rows")


def _check_b(kernel, name, kind, n, layout):
    refs = _reference(name, kind)
    out, spans, ln_bufs = _run(kernel, name, _operands(name, kind), n, layout)
    what = (kernel, name, kind, n, layout)
    _assert_unowned(out, spans, n, what)
    worst = 0.0
    for j, ((a, b), (want, ln_want, _, _)) in enumerate(zip(spans, refs)):
        got = out[:n, a:b]
        assert bool(torch.isfinite(got)[torch.isfinite(want[:n])].all()), (what, j, "non-finite output")
        r = _ratio_b(got, want[:n])
        if ln_want is not None:
            width = ln_want.shape[1]
            _assert_ln_unowned(ln_bufs[j], width, n, what)
            assert bool(torch.isfinite(ln_bufs[j][:n, :width]).all()), (what, j, "non-finite ln_out")
            r = max(r, _ratio_b(ln_bufs[j][:n, :width], ln_want[:n]))
        worst = max(worst, r)
        assert r <= 1.0, (what, "chain %d" % j, "max error / (2e-5 * max(1, max |want|))", r)
    return worst


@gpu
@pytest.mark.parametrize("kernel,name", _pairs())
def test_chain_vs_float64(kernel, name):
    """(a), (b) and the sentinel on N = 67 for every input of the launch (aligned and odd layouts in turn), then on every row
    count of SWEEP."""
    launch = _launches()[name]
    worst = {}
    for i, kind in enumerate(launch.kinds):
        worst[kind] = _check_b(kernel, name, kind, N, i % 2)
    for i, n in enumerate(SWEEP):
        worst["sweep"] = max(worst.get("sweep", 0.0), _check_b(kernel, name, launch.kinds[0], n, (i + 1) % 2))
    print("RATIO|%s|%s|%s" % (kernel, name, "|".join("%s=%.3f" % kv for kv in worst.items())))


@gpu
@pytest.mark.parametrize("kernel,name", _pairs(["lnfirst", "lnlead100", "ref2d_norm"]))
def test_ill_conditioned_layernorm_rows_vs_float64(kernel, name):
    """(a), (c) and the sentinel on offset and const rows, through a program that starts with a LayerNorm and through the
    leading LayerNorm (4-row and 32-row kernels)."""
    figures = []
    for layout, kind in enumerate(("offset", "const")):
        refs = _reference(name, kind)
        out, spans, ln_bufs = _run(kernel, name, _operands(name, kind), N, layout)
        what = (kernel, name, kind)
        _assert_unowned(out, spans, N, what)
        for j, ((a, b), (want, ln_want, fp32, ln_fp32)) in enumerate(zip(spans, refs)):
            pairs = [("out", out[:N, a:b], want, fp32)]
            if ln_want is not None:
                _assert_ln_unowned(ln_bufs[j], ln_want.shape[1], N, what)
                pairs.append(("ln_out", ln_bufs[j][:N, :ln_want.shape[1]], ln_want, ln_fp32))
            for label, got, w64, w32 in pairs:
                assert bool(torch.isfinite(got).all()), (what, j, label, "non-finite output")
                r = _ratio_c(got, w64, w32)
                figures.append("%s.%d.%s=%.3f(b:%.2f,fp32 b:%.2f)" % (kind, j, label, r, _ratio_b(got, w64), _ratio_b(w32, w64)))
                print("RATIO_C|%s|%s|%s" % (kernel, name, figures[-1]))
                assert r <= 1.0, (what, j, label, "max error / (4 e32 + 1e-7 max(1, max |want|))", r)


def _m_live_names(kernel):
    return ["w3"] + (["enc2d_sine"] if kernel != "r32" else []) + (["lnlead100", "ref2d_norm"] if kernel in ("r4", "r32") else [])


def _m_live_values(kernel):
    """The *m_live values of test_m_live_inside_and_outside_a_tile (also dumped by tools/chain_bits.py)."""
    R = KERNELS[kernel]["R"]
    return sorted({0, 1, R - 1, R, R + 1, N, 72})


@gpu
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_m_live_inside_and_outside_a_tile(kernel):
    """N = 67 with *m_live in {0, 1, R - 1, R, R + 1, 67, 72}, R the kernel's row tile: rows below it meet (b); rows of a
    workgroup that lies entirely past it are exactly 0.0; other rows past it are finite; with a leading LayerNorm ln_out is
    exactly 0.0 on every row >= m_live; rows >= N and unowned columns keep the sentinel."""
    R = KERNELS[kernel]["R"]
    for name in _m_live_names(kernel):
        kind = _launches()[name].kinds[0]
        refs = _reference(name, kind)
        for i, live in enumerate(_m_live_values(kernel)):
            out, spans, ln_bufs = _run(kernel, name, _operands(name, kind), N, i % 2, live=live)
            what = (kernel, name, "m_live", live)
            _assert_unowned(out, spans, N, what)
            rows = min(live, N)
            dead0 = min(N, -(-live // R) * R)     # first row of the first workgroup entirely past m_live
            for j, ((a, b), (want, ln_want, _, _)) in enumerate(zip(spans, refs)):
                got = out[:N, a:b]
                assert bool(torch.isfinite(got).all()), (what, j, "non-finite output")
                r = _ratio_b(got[:rows], want[:rows])
                assert r <= 1.0, (what, j, "live rows: max error / (2e-5 * max(1, max |want|))", r)
                assert bool((got[dead0:] == 0).all()), (what, j, "rows of a dead workgroup are not exactly zero")
                if ln_want is not None:
                    width = ln_want.shape[1]
                    _assert_ln_unowned(ln_bufs[j], width, N, what)
                    ln_got = ln_bufs[j][:N, :width]
                    r = _ratio_b(ln_got[:rows], ln_want[:rows])
                    assert r <= 1.0, (what, j, "ln_out live rows", r)
                    assert bool((ln_got[rows:] == 0).all()), (what, j, "ln_out is not exactly zero past m_live")


def _independence_names(kernel):
    return ["w3", "w5", "ref2d"] + (["enc2d_sine"] if kernel != "r32" else []) + (["lnlead100"] if kernel in ("r4", "r32") else [])


@gpu
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_rows_do_not_depend_on_their_neighbours(kernel):
    """(d): reverse the row order and replace every other row by other data (one with NaN, one with inf): every kept row
    comes out with the same bits at its new position. Launches without `div` (which is indexed by the row's position)."""
    g = torch.Generator().manual_seed(9)
    for name in _independence_names(kernel):
        kind = _launches()[name].kinds[0]
        ops = _operands(name, kind)
        moved = []
        for op in ops:
            x = op["x"].flip(0).clone()
            x[1::2] = 3 * torch.randn(x[1::2].shape, generator=g)
            x[1, 0], x[3, -1], x[5, 0] = float("nan"), float("inf"), float("-inf")
            post = op["post"] and dict(op["post"], res=op["post"]["res"].flip(0) if op["post"]["res"] is not None else None)
            assert not post or post["div"] is None
            moved.append(dict(x=x, x2=op["x2"].flip(0) if op["x2"] is not None else None, post=post))
        for layout in (0, 1):
            a_out, spans, a_ln = _run(kernel, name, ops, N, layout)
            b_out, _, b_ln = _run(kernel, name, moved, N, layout)
            kept = torch.arange(0, N, 2)
            for j, (a, b) in enumerate(spans):
                assert bool(torch.isfinite(a_out[:N, a:b]).all())
                assert torch.equal(b_out[kept, a:b], a_out[N - 1 - kept, a:b]), (kernel, name, layout, j, "a row changed bits")
                if a_ln[j] is not None:
                    assert torch.equal(b_ln[j][kept], a_ln[j][N - 1 - kept]), (kernel, name, layout, j, "ln_out changed bits")
