"""Float64 statement of the fp16 backbone's convolution operators (csrc/conv3x3.hip, conv1x1.hip, stem.hip, bias_act.hip),
plain torch on the CPU. It imports nothing from simpb_amd.

Maps are NHWC here: x [N, H, W, Cin], weights [Cout, kh, kw, Cin], outputs [N, Ho, Wo, Cout]. A convolution is written tap
by tap (a shifted slice of the zero-padded map times that tap's weight matrix), so one routine is the float64 statement
(`dtype=torch.float64`) and, in float32 with the kernels' 64-channel chunks, the "kernels' order" reference of the bounds.

Every operator returns a Ref:
  want     the exact statement on the operands' values, never rounded in between;
  abs_sum  the same expression on absolute values: sum |x||w| + |bias| + |residual|;
  extra    the half-ulp allowance of the rounding points IN FRONT of the output that the kernel's header documents (the
           rounded relu(x + input_bias) propagated through |w|; the stem's f16 convolution value, as the maximum over the
           pooling window); 0 where the output is the only rounding.
Bound (e) of tests/test_backbone_float64.py is  max(2^-11 |want|, 2^-25) + extra + KAPPA * 2^-24 * abs_sum."""
import collections

import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
HALF_ULP, HALF_SUBNORMAL, U24 = 2.0 ** -11, 2.0 ** -25, 2.0 ** -24
F16_MAX = 65504.0

Ref = collections.namedtuple("Ref", "want abs_sum extra")


def half_ulp(v):
    """Half an f16 ulp of a value that is rounded to f16: 2^-11 |v|, and half the subnormal quantum below that."""
    return (HALF_ULP * v.abs()).clamp_min(HALF_SUBNORMAL)


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv_taps(x, w, stride, pad, dtype=F64, chunk=64):
    """sum over taps (dy, dx) and channel chunks of x[n, ho*s + dy - pad, wo*s + dx - pad, chunk] . w[:, dy, dx, chunk]^T in
    `dtype`, taps in row-major order, chunks of a tap one after the other, each added to the running sum."""
    x, w = x.to(dtype), w.to(dtype)
    n, h, wd, c = x.shape
    co, kh, kw, _ = w.shape
    ho, wo = out_size(h, kh, stride, pad), out_size(wd, kw, stride, pad)
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    acc = torch.zeros(n, ho, wo, co, dtype=dtype)
    for dy in range(kh):
        for dx in range(kw):
            xs = xp[:, dy:dy + stride * (ho - 1) + 1:stride, dx:dx + stride * (wo - 1) + 1:stride]
            for k0 in range(0, c, chunk):
                acc = acc + xs[..., k0:k0 + chunk] @ w[:, dy, dx, k0:k0 + chunk].t()
    return acc


def conv_torch(x, w, stride, pad, dtype=F32):
    """The same convolution through torch's conv2d in `dtype` (NHWC in, NHWC out)."""
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype).permute(0, 3, 1, 2), None, stride, pad)
    return y.permute(0, 2, 3, 1).contiguous()


def up2(r):
    """Nearest 2x upsampling of an NHWC map: source = floor(dst / 2)."""
    return r.repeat_interleave(2, 1).repeat_interleave(2, 2)


def _act(v, relu):
    return v.clamp_min(0) if relu else v


def conv3x3(x, w, bias, stride=1, relu=True):
    pre = conv_taps(x, w, stride, 1) + bias.to(F64)
    ab = conv_taps(x.abs(), w.abs(), stride, 1) + bias.to(F64).abs()
    return Ref(_act(pre, relu), ab, torch.zeros_like(ab))


def conv1x1(x, w, bias, residual=None, relu=True, stride=1, residual_upsample2x=False, input_bias=None):
    """w [Cout, Cin]. residual [N, Ho, Wo, Cout], or half that size with residual_upsample2x."""
    w4 = w.reshape(w.shape[0], 1, 1, w.shape[1])
    a = x.to(F64)
    extra = None
    if input_bias is not None:
        a = (a + input_bias.to(F64)).clamp_min(0)
        extra = conv_taps(half_ulp(a) * (a > 0), w4.abs(), stride, 0)   # relu(.) = 0 is stored exactly
    pre = conv_taps(a, w4, stride, 0) + bias.to(F64)
    ab = conv_taps(a.abs(), w4.abs(), stride, 0) + bias.to(F64).abs()
    if residual is not None:
        r = up2(residual.to(F64)) if residual_upsample2x else residual.to(F64)
        pre, ab = pre + r, ab + r.abs()
    return Ref(_act(pre, relu), ab, extra if extra is not None else torch.zeros_like(ab))


def max_pool(v, pad_value=-float("inf")):
    """max-pool 3x3 / 2 / pad 1 of an NHWC map with `pad_value` outside."""
    vp = F.pad(v, (0, 0, 1, 1, 1, 1), value=pad_value)
    n, h, w, c = v.shape
    ho, wo = out_size(h, 3, 2, 1), out_size(w, 3, 2, 1)
    out = torch.full((n, ho, wo, c), pad_value, dtype=v.dtype)
    for dy in range(3):
        for dx in range(3):
            out = torch.maximum(out, vp[:, dy:dy + 2 * (ho - 1) + 1:2, dx:dx + 2 * (wo - 1) + 1:2])
    return out


def stem(img, w, bias):
    """img [N, H, W, 3] (f16 values), w [64, 7, 7, 3]: maxpool3x3/2/1(relu(conv7x7/2/3 + bias)), the pool's padding -inf.
    |max a - max b| <= max |a - b|: the allowances of a pooled element are the maxima of its window's."""
    conv = conv_taps(img, w, 2, 3, chunk=3)
    ab = conv_taps(img.abs(), w.abs(), 2, 3, chunk=3) + bias.to(F64).abs()
    want = max_pool((conv + bias.to(F64)).clamp_min(0), -float("inf"))
    return Ref(want, max_pool(ab, -float("inf")), max_pool(half_ulp(conv), -float("inf")))


def bias_act(y, bias, residual=None, relu=True):
    pre, ab = y.to(F64) + bias.to(F64), y.to(F64).abs() + bias.to(F64).abs()
    if residual is not None:
        pre, ab = pre + residual.to(F64), ab + residual.to(F64).abs()
    return Ref(_act(pre, relu), ab, torch.zeros_like(ab))


def bias_relu_maxpool(x, bias):
    v = x.to(F64) + bias.to(F64)
    return Ref(max_pool(v.clamp_min(0), -float("inf")), max_pool(x.to(F64).abs() + bias.to(F64).abs(), -float("inf")),
               torch.zeros_like(max_pool(v, -float("inf"))))


def token_rows(levels, bs, cams, per_cam, starts):
    """The decoder's token layout by hand: levels = [[bs * cams, H_j, W_j, C] per level] -> (rows [bs, cams * per_cam, C] with
    NaN where no level writes, written [bs, cams * per_cam] bool): pixel (h, w) of level j of image b * cams + cam is row
    cam * per_cam + starts[j] + h * W_j + w of stream b."""
    c = levels[0].shape[-1]
    rows = torch.full((bs, cams * per_cam, c), float("nan"), dtype=levels[0].dtype)
    written = torch.zeros(bs, cams * per_cam, dtype=torch.bool)
    for lvl, start in zip(levels, starts):
        n, h, w, _ = lvl.shape
        assert n == bs * cams and start >= 0 and start + h * w <= per_cam
        for b in range(bs):
            for cam in range(cams):
                r0 = cam * per_cam + start
                assert not written[b, r0:r0 + h * w].any()
                rows[b, r0:r0 + h * w] = lvl[b * cams + cam].reshape(h * w, c)
                written[b, r0:r0 + h * w] = True
    return rows, written


# ------------------------------------------------------------------------------------------------- float32 references
def round_f16(v):
    return v.to(torch.float16)


def conv_f32(x, w, stride, pad, order, chunk=64):
    """order "torch": conv2d in float32; "taps": the kernels' order (conv_taps in float32)."""
    return conv_torch(x, w, stride, pad) if order == "torch" else conv_taps(x, w, stride, pad, F32, chunk)


def finish_f32(v, relu):
    """The epilogue's last step on an fp32 pre-activation value: ReLU, one rounding to f16."""
    return round_f16(_act(v, relu))


def conv3x3_pre32(x, w, bias, stride, order):
    return conv_f32(x, w, stride, 1, order) + bias.to(F32)


def conv3x3_f32(x, w, bias, stride, relu, order):
    return finish_f32(conv3x3_pre32(x, w, bias, stride, order), relu)


def conv1x1_pre32(x, w, bias, residual, stride, residual_upsample2x, input_bias, order):
    a = x.to(F32)
    if input_bias is not None:
        a = round_f16((a + input_bias.to(F32)).clamp_min(0)).to(F32)
    v = conv_f32(a, w.reshape(w.shape[0], 1, 1, w.shape[1]), stride, 0, order) + bias.to(F32)
    if residual is not None:
        v = v + (up2(residual.to(F32)) if residual_upsample2x else residual.to(F32))
    return v


def conv1x1_f32(x, w, bias, residual, relu, stride, residual_upsample2x, input_bias, order):
    return finish_f32(conv1x1_pre32(x, w, bias, residual, stride, residual_upsample2x, input_bias, order), relu)


def stem_f32(img, w, bias, order):
    conv = round_f16(conv_f32(img, w, 2, 3, order, chunk=3)).to(F32)
    return round_f16(max_pool((conv + bias.to(F32)).clamp_min(0), -float("inf")))


def bias_act_f32(y, bias, residual, relu):
    v = y.to(F32) + bias.to(F32)
    if residual is not None:
        v = v + residual.to(F32)
    return round_f16(_act(v, relu))


def bias_relu_maxpool_f32(x, bias):
    return round_f16(max_pool((x.to(F32) + bias.to(F32)).clamp_min(0), -float("inf")))


# ----------------------------------------------------------------------------------------------------------------- bounds
def bound_e(ref, kappa):
    return half_ulp(ref.want) + ref.extra + kappa * U24 * ref.abs_sum


def figure_e(got, ref, kappa, judged=None):
    """Largest |got - want| / bound (e) over the judged elements (1.0 = on the bound); inf - inf counts as inf."""
    err = (got.to(F64) - ref.want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    fig = err / bound_e(ref, kappa)
    if judged is not None:
        fig = fig[judged]
    return float(fig.max()) if fig.numel() else 0.0


def kappa_needed(got, ref):
    """The smallest kappa that covers what a reference's fp32 arithmetic adds to its own roundings, on every finite element:
    |got - want| <= half_ulp + extra + kappa * 2^-24 * abs_sum. (A reference that rounds its result to f16 uses the rounding
    terms of (e) in full whatever its arithmetic: `half of the bound` can only be asked of the kappa term.)"""
    ok = torch.isfinite(got.to(F64)) & (ref.want.abs() <= F16_MAX)
    over = ((got.to(F64) - ref.want).abs() - (half_ulp(ref.want) + ref.extra))[ok]
    ab = ref.abs_sum[ok]
    if bool(((over > 0) & (ab == 0)).any()):
        return float("inf")
    k = torch.where(over > 0, over / (U24 * ab.clamp_min(1e-300)), torch.zeros_like(over))
    return float(k.max()) if k.numel() else 0.0
