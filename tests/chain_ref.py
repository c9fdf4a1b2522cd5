"""Plain PyTorch statement of one chain program of simpb_mlp_chain_forward (include/simpb_hip.h, csrc/mlp_chain.hip), in a
chosen dtype: float64 is the reference of tests/test_mlp_chain_float64.py, float32 is its "plain fp32" baseline."""
import math

import torch
import torch.nn as nn

POST_NONE, POST_REFINE3D, POST_REFINE2D, POST_SIGMOID = 0, 1, 2, 3   # SIMPB_MLP_POST_*


def chain_ref(seq, x, x2=None, sine=False, ln=None, post=None, dtype=torch.float64):
    """(out, ln_out) of one chain over the rows of x [N, in_dim], every operand cast to `dtype` first.

    seq   nn.Sequential of Linear (an nn.ReLU behind it is the op's relu flag), LayerNorm and a trailing Scale (any module
          with a `.scale` parameter); only its parameters are read, every formula is written out here.
    input x (+ x2); sine: x holds (x, y) at columns 0, 1 and the input is pos2posemb2d (models/utils.py:40-63): 128 features
          of y, then 128 of x, feature i = sin (even i) or cos (odd i) of coord * 2 pi / 10000^(2 (i // 2) / 128). The
          divisor table is a float32 constant there (arange and power in float32), so it is one here, in every dtype;
          ln (an nn.LayerNorm over in_dim): input = LN(x) + x2, and ln_out = LN(x) is returned (None without ln).
    LayerNorm: (v - mean) / sqrt(biased variance + 1e-5) * gamma + beta.
    post  None or dict(kind, res=[N, >= res_cols], res_cols, div=[batches] or None, div_rows, div_col0), applied to v =
          out[row, t] after the Scale:
          POST_REFINE3D  t >= div_col0: v / div[row // div_rows]; then t < res_cols: v + res[row, t]
          POST_REFINE2D  t < res_cols: v + inverse_sigmoid(clamp(res[row, t], 0, 1), eps 1e-5); then sigmoid(v)
          POST_SIGMOID   sigmoid(v)"""
    def c(t):
        return t.detach().to(device="cpu", dtype=dtype)

    def layernorm(v, m):
        mean = v.mean(-1, keepdim=True)
        var = ((v - mean) ** 2).mean(-1, keepdim=True)
        return (v - mean) / torch.sqrt(var + 1e-5) * c(m.weight) + c(m.bias)

    v = c(x)
    ln_out = None
    if sine:
        dim_t = torch.arange(128, dtype=torch.float32)
        dim_t = (10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / 128)).to(dtype)
        feats = []
        for col in (1, 0):
            p = (v[:, col] * (2 * math.pi))[:, None] / dim_t
            feats.append(torch.stack((p[:, 0::2].sin(), p[:, 1::2].cos()), dim=-1).flatten(-2))
        v = torch.cat(feats, dim=-1)
    elif ln is not None:
        v = ln_out = layernorm(v, ln)
    if x2 is not None:
        v = v + c(x2)
    for m in seq:
        if isinstance(m, nn.Linear):
            v = v @ c(m.weight).t()
            if m.bias is not None:
                v = v + c(m.bias)
        elif isinstance(m, nn.ReLU):
            v = v.clamp(min=0)
        elif isinstance(m, nn.LayerNorm):
            v = layernorm(v, m)
        elif hasattr(m, "scale"):
            v = v * c(m.scale)
        else:
            raise ValueError(type(m).__name__)
    if post is not None and post["kind"] != POST_NONE:
        n, width = v.shape
        if post["kind"] == POST_REFINE3D:
            if post.get("div") is not None:
                d = c(post["div"])[torch.arange(n) // post["div_rows"]][:, None]
                v = torch.cat([v[:, :post["div_col0"]], v[:, post["div_col0"]:] / d], dim=-1)
            k = min(post["res_cols"], width)
            v = torch.cat([v[:, :k] + c(post["res"])[:, :k], v[:, k:]], dim=-1)
        elif post["kind"] == POST_REFINE2D:
            k = min(post["res_cols"], width)
            a = c(post["res"])[:, :k].clamp(min=0, max=1)
            inv = torch.log(a.clamp(min=1e-5) / (1 - a).clamp(min=1e-5))
            v = torch.sigmoid(torch.cat([v[:, :k] + inv, v[:, k:]], dim=-1))
        elif post["kind"] == POST_SIGMOID:
            v = torch.sigmoid(v)
        else:
            raise ValueError(post["kind"])
    return v, ln_out
