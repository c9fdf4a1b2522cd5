"""Host side of csrc/gemm.hip: the decoder's query-sized nn.Linear layers as grouped, segment-input
GEMM launches, the segmented LayerNorm, and the weight folds that turn the reference's chains of
linear maps into single products:

  * graph_model (simpb_head.py:298-310): value = in_proj_v(fc_before(v))  ->  one map W_v.W_fb
    out = fc_after(cat(q, pos) + out_proj(o))  ->  [o | q | pos] . [W_a.W_o | W_a]^T + W_a.b_o
  * AsymmetricFFN (blocks.py:384-393): identity_fc(x) + fc2(relu(fc1(x)))  ->  [h | x] . [W_2 | W_id]^T + b_2 + b_id

Folding only re-associates fp32 sums (differences ~1e-6 relative, covered by the operator tests);
the module tree and the state_dict are untouched, and the folded copies are rebuilt whenever a
parameter is replaced or modified in place. GPU only: there is no CPU path behind these calls."""
import ctypes
import math
import warnings

import torch

from .. import _lib
from .ops import _stream

MAX_SEGS, MAX_JOBS = 4, 4

# routes.dense: the decoder's query-sized Linear layers go through csrc/gemm.hip (grouped, segment-input GEMMs with
# host-folded weights). Off: one GEMM per nn.Linear plus the cat/add kernels around it, where every module boundary of
# the reference exists -- kept for A/B measurements and as the route on which tests/test_gpu_head.py compares every
# golden trace record.
# routes.gemm_split_fp16 (shipped since round 4): weights are also handed over split into two half-precision parts, and
# launches whose segments are 128-aligned run on the FP16 matrix cores in four split passes (csrc/gemm.hip:
# gemm_f16x3_kernel: every partial product of x = xh + xl / 2^11 and W = Wh + Wl / 2^11, fp32 accumulators). Measured
# against float64 on the decoder's shapes its error is about HALF that of the exact-fp32 matrix-core kernel
# (profiles/r04_gemm_split_error.txt), tests/test_dense.py holds both to the same bound, and every golden / oracle / runner
# test is green on it; -0.09 ms on the decoder's critical path. Off: always the v_mfma_f32_32x32x2_f32 kernel. Any
# re-rounding CAN move a 2D query across an image border (~1e-6 of the 583k point tests of a stream fall within rounding
# distance of one; a three-term form of this kernel did so on the golden R50 stream in round 1): what the golden vectors pin
# is that this form does not on any fixture, not that it cannot.
from . import routes


# Rows of W whose largest |w| lies in this window (or that are all zeros) split into two halfs with 22 bits relative to
# the row; outside it half(w) overflows (|w| >= 65520) or the row falls into the half subnormals. The GEMM kernels handle
# rows of x outside it themselves (csrc/gemm.hip split_row_outside: same window).
SPLIT_WINDOW = (2.0 ** -10, 2.0 ** 15)


def split_in_window(w):
    """True when every row of w [N, K] has its largest |w| inside SPLIT_WINDOW or is all zeros (and nothing is inf / NaN):
    the weights the split-operand kernels take. One device-to-host read per weight; callers cache the answer."""
    if w.numel() == 0:
        return True
    m = w.detach().abs().amax(dim=-1).double().cpu()
    ok = bool(torch.isfinite(m).all()) and bool(((m == 0) | ((m >= SPLIT_WINDOW[0]) & (m < SPLIT_WINDOW[1]))).all())
    if not ok and not getattr(split_in_window, "_warned", False):
        split_in_window._warned = True
        warnings.warn("simpb_amd: a weight has rows outside the split-operand window "
                      f"[{SPLIT_WINDOW[0]:g}, {SPLIT_WINDOW[1]:g}); its launches run on the exact-fp32 kernel")
    return ok


def _split_weights(w):
    """(w_hi, w_lo) f16 [N, K] of a contiguous f32 weight: w = w_hi + w_lo / 2048 up to ~2^-22 relative; (None, None)
    for a weight outside the split window (split_in_window): its launches take the exact-fp32 kernel. Cached ON
    the tensor object (not in a table keyed by address or id(): both are reused once a model is freed)."""
    tag = (w.data_ptr(), w._version, str(w.device))
    hit = getattr(w, "_simpb_split", None)
    if hit is None or hit[0] != tag:
        if torch.cuda.is_current_stream_capturing():
            return None, None   # no host read inside a capture: a weight first seen there takes the exact kernel
        if split_in_window(w):
            with torch.no_grad():
                hi = w.detach().half()
                lo = ((w.detach() - hi.float()) * 2048.0).half()
            hit = (tag, hi.contiguous(), lo.contiguous())
        else:
            hit = (tag, None, None)
        w._simpb_split = hit
    return hit[1], hit[2]


class _Job(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p * MAX_SEGS), ("ldx", ctypes.c_int * MAX_SEGS), ("kseg", ctypes.c_int * MAX_SEGS),
                ("num_seg", ctypes.c_int), ("M", ctypes.c_int), ("N", ctypes.c_int), ("K", ctypes.c_int),
                ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p), ("m_live", ctypes.c_void_p),
                ("ldw", ctypes.c_int), ("ldy", ctypes.c_int), ("relu", ctypes.c_int), ("out_fmt", ctypes.c_int),
                ("row_flag", ctypes.c_void_p), ("bias2", ctypes.c_void_p), ("w_hi", ctypes.c_void_p), ("w_lo", ctypes.c_void_p)]


class _Args(ctypes.Structure):
    _fields_ = [("num_jobs", ctypes.c_int), ("reserved", ctypes.c_int), ("job", _Job * MAX_JOBS)]


class Segments(list):
    """A row-wise concatenation that has not been materialised: [t0 | t1 | ...] along the last
    dimension. The deformable operators return one under residual_mode="cat" when the consumer (the
    FFN's pre-norm) can read the parts in place."""

    def materialize(self):
        return torch.cat(list(self), dim=-1)

    @property
    def shape(self):
        return self[0].shape[:-1] + (sum(t.shape[-1] for t in self),)


def report(module, out):
    """Hand `out` to the forward hooks registered on `module`. A fused block computes the value a
    reference module boundary would have produced (fc_after, a `norm` op) without calling that
    module, so this is how the per-operator parity traces (tests/helpers.py:attach_trace_hooks)
    still see it. No hooks registered (the product path): a dict lookup."""
    hooks = getattr(module, "_forward_hooks", None)
    if hooks:
        for hook in list(hooks.values()):
            hook(module, (), out)
    return out


def rows2d(t):
    """(tensor to take the pointer from, number of rows, row stride) for [..., k] with unit inner
    stride and a uniform row stride; anything else is made contiguous first."""
    if t.dtype != torch.float32:
        t = t.float()
    k = t.shape[-1]
    ok = t.stride(-1) == 1 or k == 1
    ld = None
    if ok:
        span = 1
        for size, stride in zip(reversed(t.shape[:-1]), reversed(t.stride()[:-1])):
            if size == 1:
                continue
            if ld is None:
                ld = stride
            elif stride != ld * span:
                ok = False
                break
            span *= size
        if ld is None:
            ld = k
    if not ok or ld < k or ld % 4 or t.data_ptr() % 16:
        t = t.contiguous()
        ld = k
    rows = 1
    for s in t.shape[:-1]:
        rows *= s
    return t, rows, ld


def job(xs, w, bias=None, relu=False, out=None, m_live=None, row_flag=None, bias2=None, split_halfs=False):
    """One problem of a grouped launch: y = relu?([xs...] . w^T + bias [+ bias2 on rows whose
    row_flag != 0]). xs: tensor or list of tensors sharing their leading dimensions; w [N, K] (a row
    slice of a larger matrix is fine); out: optional destination [..., N] view (e.g. a column range
    of a wider buffer); row_flag i32 [rows], bias2 f32 [N]."""
    if torch.is_tensor(xs):
        xs = [xs]
    return dict(xs=list(xs), w=w, bias=bias, relu=relu, out=out, m_live=m_live, row_flag=row_flag, bias2=bias2,
                split_halfs=split_halfs)


def gemm(*jobs):
    """Run up to 4 jobs in one launch; returns their outputs (shaped like the inputs' leading
    dimensions + [N])."""
    if not 1 <= len(jobs) <= MAX_JOBS:
        raise ValueError("1..4 jobs per launch")
    args = _Args()
    args.num_jobs = len(jobs)
    keep, outs = [], []
    for j, spec in enumerate(jobs):
        jb = args.job[j]
        w = spec["w"]
        if not w.is_cuda:
            raise RuntimeError("simpb_amd GEMMs run on the GPU only (no CPU path)")
        if w.dtype != torch.float32 or w.stride(1) != 1:
            w = w.float().contiguous()
        n, k = w.shape
        lead = spec["xs"][0].shape[:-1]
        m = None
        ksum = 0
        if len(spec["xs"]) > MAX_SEGS:
            raise ValueError("at most 4 column segments")
        for s, x in enumerate(spec["xs"]):
            xt, rows, ld = rows2d(x)
            if m is None:
                m = rows
            elif rows != m:
                raise ValueError("segments disagree on the number of rows")
            jb.x[s], jb.ldx[s], jb.kseg[s] = xt.data_ptr(), ld, x.shape[-1]
            ksum += x.shape[-1]
            keep.append(xt)
        if ksum != k:
            raise ValueError(f"segment widths sum to {ksum}, weight has K={k}")
        out = spec["out"]
        if out is None:
            out = torch.empty(lead + (n,), device=w.device, dtype=torch.float32)
        ot, orows, ldo = rows2d(out)
        if ot is not out and ot.data_ptr() != out.data_ptr():
            raise ValueError("output view must have unit inner stride and uniform, 16-byte aligned rows")
        if orows != m or out.shape[-1] != n:
            raise ValueError("output shape mismatch")
        bias = spec["bias"]
        if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
            bias = bias.float().contiguous()
        jb.num_seg, jb.M, jb.N, jb.K = len(spec["xs"]), m, n, k
        jb.w, jb.ldw = w.data_ptr(), w.stride(0)
        if routes.R.gemm_split_fp16 and w.is_contiguous() and all(x.shape[-1] % 128 == 0 for x in spec["xs"]):
            w_hi, w_lo = _split_weights(w)
            if w_hi is not None:
                jb.w_hi, jb.w_lo = w_hi.data_ptr(), w_lo.data_ptr()
                keep += [w_hi, w_lo]
        jb.bias = bias.data_ptr() if bias is not None else None
        jb.y, jb.ldy = out.data_ptr(), ldo
        jb.relu = 1 if spec["relu"] else 0
        # split_halfs: every output element as the (hi, lo) half pair of csrc/attention.hip's split-operand kernel, in
        # the element's own 32-bit word (the tensor is fp32-typed storage of those words: only that kernel reads it)
        jb.out_fmt = 1 if spec.get("split_halfs") else 0
        ml = spec["m_live"]
        jb.m_live = ml.data_ptr() if ml is not None else None
        rf, b2 = spec.get("row_flag"), spec.get("bias2")
        if (rf is None) != (b2 is None):
            raise ValueError("row_flag and bias2 go together")
        if rf is not None:
            if rf.dtype != torch.int32 or not rf.is_contiguous() or rf.numel() != m or b2.numel() != n:
                raise ValueError("row_flag must be contiguous i32 [rows], bias2 f32 [N]")
            b2 = b2.float().contiguous()
            jb.row_flag, jb.bias2 = rf.data_ptr(), b2.data_ptr()
        keep += [w, bias, out, ml, rf, b2]
        outs.append(out)
    if any(o.numel() for o in outs):
        _lib.check(_lib.lib().simpb_gemm_f32(ctypes.byref(args), _stream()), "simpb_gemm_f32")
    return outs


def linear(xs, w, bias=None, relu=False, out=None, m_live=None, row_flag=None, bias2=None, split_halfs=False):
    return gemm(job(xs, w, bias, relu, out, m_live, row_flag, bias2, split_halfs))[0]


def rowdot_sigmoid(x, w, b, m_live=None):
    """sigmoid(x . w + b) per row: x [..., k], w [1, k] or [k], b [1] -> [..., 1]."""
    xt, rows, ld = rows2d(x)
    out = torch.empty(x.shape[:-1] + (1,), device=x.device, dtype=torch.float32)
    w = w.reshape(-1).float().contiguous()
    if rows:
        _lib.check(_lib.lib().simpb_rowdot_sigmoid(out.data_ptr(), xt.data_ptr(), ld, w.data_ptr(),
                                                   b.data_ptr() if b is not None else None, rows, x.shape[-1],
                                                   m_live.data_ptr() if m_live is not None else None, _stream()),
                   "simpb_rowdot_sigmoid")
    return out


def layernorm(xs, ln, out=None, m_live=None):
    """LayerNorm over cat(xs) (one or two segments) with the affine of `ln` (nn.LayerNorm)."""
    if torch.is_tensor(xs):
        xs = [xs]
    if len(xs) > 2 or abs(ln.eps - 1e-5) > 1e-12:
        raise ValueError("layernorm: one or two segments, eps 1e-5")
    x0, m, ld0 = rows2d(xs[0])
    k0 = xs[0].shape[-1]
    x1, ld1, k1 = None, 0, 0
    if len(xs) == 2:
        x1, m1, ld1 = rows2d(xs[1])
        k1 = xs[1].shape[-1]
        if m1 != m:
            raise ValueError("segments disagree on the number of rows")
    d = k0 + k1
    if ln.normalized_shape != (d,) or not x0.is_cuda:
        raise ValueError("layernorm width mismatch or CPU tensor")
    if out is None:
        out = torch.empty(xs[0].shape[:-1] + (d,), device=x0.device, dtype=torch.float32)
    _, _, ldo = rows2d(out)
    if m:
        _lib.check(_lib.lib().simpb_layernorm_f32(
            out.data_ptr(), ldo, x0.data_ptr(), ld0, k0, x1.data_ptr() if x1 is not None else None, ld1, k1,
            ln.weight.data_ptr(), ln.bias.data_ptr(), m, m_live.data_ptr() if m_live is not None else None,
            _stream()), "simpb_layernorm_f32")
    return report(ln, out)


# ---------------------------------------------------------------------------- weight folds
class FoldCache:
    """Derived weights, stored ON the module that owns the leading parameter (`owner`) and tagged with the
    address and version of every parameter they were built from. Not a global table keyed by id(): ids and
    device addresses are reused once a model is freed, and a second model would pick up the first one's folds."""

    def get(self, key, params, build, owner=None):
        tag = tuple((p.data_ptr(), p._version, str(p.device)) if p is not None else None for p in params)
        owner = owner if owner is not None else next(p for p in params if p is not None)
        store = owner.__dict__.setdefault("_simpb_folds", {}) if hasattr(owner, "__dict__") else None
        if store is None:
            with torch.no_grad():
                return build()
        hit = store.get(key)
        if hit is None or hit[0] != tag:
            with torch.no_grad():
                hit = (tag, build())
            store[key] = hit
        return hit[1]


_folds = FoldCache()


def _f64(t):
    return t.detach().double()


def fold_mha_in(attn, pre, mode, q_scale=None):
    """Input side of an nn.MultiheadAttention fed with query = cat(f, pos) (E = 2 C wide) and
    value = pre(f) (pre = fc_before [E, C], no bias) or the query itself (pre None).
    mode 'qkv': rows [q; k; v] over [f | pos]; 'q': rows [q]; 'kv': rows [k; v].
    q_scale: the softmax scale folded into the query rows (weight and bias), for the attention kernel that takes
    pre-split operands (a power of two -- 1 / sqrt(64) -- so the projected queries are bit for bit scale * q).
    Returns (weight [rows, E], bias [rows])."""
    w, b = attn.in_proj_weight, attn.in_proj_bias
    e = attn.embed_dim
    if q_scale is not None and (q_scale <= 0 or math.frexp(q_scale)[0] != 0.5):
        raise ValueError("q_scale must be a power of two (folded exactly)")

    def build():
        if pre is None:
            wv = _f64(w[2 * e:])
        else:
            c = pre.weight.shape[1]
            wv = torch.cat([_f64(w[2 * e:]) @ _f64(pre.weight), torch.zeros(e, e - c, dtype=torch.float64, device=w.device)], 1)
        parts = {"qkv": [_f64(w[:e]), _f64(w[e: 2 * e]), wv], "q": [_f64(w[:e])], "kv": [_f64(w[e: 2 * e]), wv]}[mode]
        bias = {"qkv": b, "q": b[:e], "kv": b[e:]}[mode].detach().float().clone()
        weight = torch.cat(parts, 0).float().contiguous()
        if q_scale is not None and mode in ("qkv", "q"):
            weight[:e] *= q_scale
            bias[:e] *= q_scale
        return weight, bias.contiguous()

    return _folds.get(("mha_in", mode, pre is not None, q_scale), (w, b, pre.weight if pre is not None else None), build, owner=attn)


def fold_mha_out(attn, post):
    """Output side: post(identity + out_proj(o)) with identity = cat(f, pos) and post = fc_after
    [C, E] (no bias) -> weight [C, 2 E] over [o | f | pos], bias [C]."""
    wo, bo = attn.out_proj.weight, attn.out_proj.bias

    def build():
        wa = _f64(post.weight)
        weight = torch.cat([wa @ _f64(wo), wa], 1).float().contiguous()
        bias = (wa @ _f64(bo)).float().contiguous()
        return weight, bias

    return _folds.get(("mha_out",), (wo, bo, post.weight), build, owner=attn)


def fold_ffn_out(fc2, identity_fc):
    """[h | x] . [W_2 | W_id]^T + b_2 + b_id."""

    def build():
        weight = torch.cat([fc2.weight.detach(), identity_fc.weight.detach()], 1).float().contiguous()
        bias = (fc2.bias.detach() + identity_fc.bias.detach()).float().contiguous()
        return weight, bias

    return _folds.get(("ffn_out",), (fc2.weight, fc2.bias, identity_fc.weight, identity_fc.bias), build, owner=fc2)


def fold_msda_linear(value_proj, output_proj, heads, width):
    """QueryGroupMultiScaleDeformableAttention with value_proj moved behind the sampling (csrc/msda_lin.hip): the map from
    agg = [per head: 256 sampled-token sums | per head: tap-weight sum | pad] to output_proj(concat_h(W_h agg_h + b_h s_h)):
    weight [C, width], columns [h*256, (h+1)*256) = W_o[:, head h] . W_v[head h, :], column 8*256 + h = W_o[:, head h] . b_v[head h];
    bias = b_o. float64 fold."""

    def build():
        wv, bv = _f64(value_proj.weight), _f64(value_proj.bias)
        wo = _f64(output_proj.weight)
        c = wv.shape[1]
        hd = wv.shape[0] // heads
        out = torch.zeros(wo.shape[0], width, dtype=torch.float64, device=wo.device)
        for h in range(heads):
            blk = wo[:, h * hd:(h + 1) * hd]
            out[:, h * c:(h + 1) * c] = blk @ wv[h * hd:(h + 1) * hd]
            out[:, heads * c + h] = blk @ bv[h * hd:(h + 1) * hd]
        return out.float().contiguous(), output_proj.bias.detach().float().contiguous()

    return _folds.get(("msda_linear", heads, width), (value_proj.weight, value_proj.bias, output_proj.weight, output_proj.bias),
                      build, owner=value_proj)


def fold_split_last_column(lin):
    """A Linear over cat(x, flag) with a 0/1 flag column: (weight over x [N, K-1] with 16-byte aligned
    rows, column of the flag [N])."""

    def build():
        w = lin.weight.detach().float()
        return w[:, :-1].contiguous(), w[:, -1].contiguous()

    return _folds.get(("split_last",), (lin.weight,), build, owner=lin)


def fold_sum_input(lin, copies=2):
    """lin(a + b) = [a | b] . [W | W]^T + bias."""

    def build():
        return torch.cat([lin.weight.detach()] * copies, 1).float().contiguous()

    return _folds.get(("sum_in", copies), (lin.weight,), build, owner=lin)


def fold_stack(key, linears, copies=1):
    """Several Linear layers over the same input stacked along N: ([W_0; W_1; ...] each repeated
    `copies` times along K, cat of biases)."""

    def build():
        weight = torch.cat([torch.cat([m.weight.detach()] * copies, 1) for m in linears], 0).float().contiguous()
        bias = torch.cat([m.bias.detach() for m in linears], 0).float().contiguous()
        return weight, bias

    params = tuple(p for m in linears for p in (m.weight, m.bias))
    return _folds.get((key, copies, len(linears)), params, build, owner=linears[0])
