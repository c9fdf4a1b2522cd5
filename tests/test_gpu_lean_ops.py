"""GPU: the two native pieces a replayed frame runs instead of today's (profiles/lean_frames.md).

(a) csrc/conv3x3.hip with tokens == NULL and tokens_f16 set: the FPN's output convolution writes the f16 token rows alone.
    Against the two-copy call (fp32 + f16 rows): the f16 rows are bit-equal, and nothing outside them is written (the f16
    buffer sits between sentinel-filled guard rows). 2 images x 2 cameras, two levels (8 x 12 and 4 x 6), Cin = 64,
    Cout = 64 (whole 16-byte pieces) and Cout = 72 (the last channel block takes the tail path); the single-level entry at
    every tiling (each is its own kernel) and the grouped entry.
(b) csrc/mlp_chain.hip with a job that is the leading LayerNorm stage alone (no chain, no `out`): its ln_out against the
    ln_out of the same job with a real chain behind it, bit for bit, in the 4-row kernel (N = 5: a partial last workgroup)
    and the 32-row kernel (N = 33), with m_live in {none, 3, 0} (3: the cut falls inside a workgroup; rows at and past it
    are zeros)."""
import ctypes

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

SENT16 = -1234.0   # exactly representable in f16; no convolution result here comes near it
SENT = -7.25e6
BS, CAMS, CIN = 2, 2, 64
LEVELS = ((8, 12), (4, 6))
PER_CAM = sum(h * w for h, w in LEVELS)
STARTS = (0, LEVELS[0][0] * LEVELS[0][1])
GUARD = 3          # rows in front of and behind the token rows


def _conv_operands(cout):
    g = torch.Generator().manual_seed(17 + cout)
    xs = [torch.randn(BS * CAMS, CIN, h, w, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
          for h, w in LEVELS]
    ws = [(torch.randn(cout, CIN, 3, 3, generator=g) / 24).half().cuda().contiguous(memory_format=torch.channels_last)
          for _ in LEVELS]
    bs_ = [torch.randn(cout, generator=g).half().cuda() for _ in LEVELS]
    return xs, ws, bs_


def _guarded(cout):
    """(whole buffer [GUARD + rows + GUARD, cout], the token rows [BS, CAMS * PER_CAM, cout] as a view of it), sentinel-filled."""
    rows = BS * CAMS * PER_CAM
    whole = torch.full((rows + 2 * GUARD, cout), SENT16, dtype=torch.float16, device="cuda")
    return whole, whole[GUARD:GUARD + rows].view(BS, CAMS * PER_CAM, cout)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_f16_only(whole, col16, want16, want32, what):
    torch.cuda.synchronize()
    assert torch.equal(_bits(col16), _bits(want16)), (what, "f16 rows differ from the two-copy call's")
    assert torch.equal(col16.float(), want32), (what, "f16 rows are not the fp32 rows' numbers")
    assert not bool((col16 == SENT16).any()), (what, "a token row was left unwritten")
    assert bool((whole[:GUARD] == SENT16).all()) and bool((whole[-GUARD:] == SENT16).all()), (what, "written outside the token rows")


@pytest.mark.parametrize("cout", [64, 72])
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_single_level_entry_writes_the_f16_rows_alone(cout, variant):
    from simpb_amd.plugin import ops
    xs, ws, bs_ = _conv_operands(cout)
    want32 = torch.full((BS, CAMS * PER_CAM, cout), SENT, device="cuda")
    want16 = torch.full((BS, CAMS * PER_CAM, cout), SENT16, dtype=torch.float16, device="cuda")
    whole, col16 = _guarded(cout)
    for j in range(len(LEVELS)):
        ops.conv3x3_nhwc(xs[j], ws[j], bs_[j], relu=False, tokens=(want32, PER_CAM, STARTS[j], want16), variant=variant)
        ops.conv3x3_nhwc(xs[j], ws[j], bs_[j], relu=False, tokens=(None, PER_CAM, STARTS[j], col16), variant=variant)
    _check_f16_only(whole, col16, want16, want32, ("single", cout, variant))


@pytest.mark.parametrize("cout", [64, 72])
def test_grouped_entry_writes_the_f16_rows_alone(cout):
    from simpb_amd.plugin import ops
    xs, ws, bs_ = _conv_operands(cout)
    want32 = torch.full((BS, CAMS * PER_CAM, cout), SENT, device="cuda")
    want16 = torch.full((BS, CAMS * PER_CAM, cout), SENT16, dtype=torch.float16, device="cuda")
    whole, col16 = _guarded(cout)
    ops.conv3x3_group_tokens(xs, ws, bs_, want32, PER_CAM, list(STARTS), want16)
    ops.conv3x3_group_tokens(xs, ws, bs_, None, PER_CAM, list(STARTS), col16)
    _check_f16_only(whole, col16, want16, want32, ("grouped", cout))


def test_no_output_at_all_is_still_refused():
    from simpb_amd import _lib
    from simpb_amd.plugin.ops import _ptr, _stream
    xs, ws, bs_ = _conv_operands(64)
    h, w = LEVELS[0]
    lib = _lib.lib()
    status = lib.simpb_conv3x3_nhwc_f16(None, None, None, PER_CAM, 0, _ptr(xs[0]), _ptr(ws[0]), _ptr(bs_[0]), BS * CAMS, h, w,
                                        CIN, 64, 1, 0, 0, _stream())
    assert status == 1   # SIMPB_EINVAL
    k = len(LEVELS)
    arr_p, arr_i = ctypes.c_void_p * k, ctypes.c_int * k
    status = lib.simpb_conv3x3_group_tokens_f16(
        k, None, None, PER_CAM, arr_i(*STARTS), arr_p(*[x.data_ptr() for x in xs]), arr_p(*[x.data_ptr() for x in ws]),
        arr_p(*[x.data_ptr() for x in bs_]), BS * CAMS, arr_i(*[h for h, _ in LEVELS]), arr_i(*[w for _, w in LEVELS]), CIN, 64,
        0, _stream())
    assert status == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (b) LayerNorm-only job
D = 256


def _chain_operands(n):
    from simpb_amd.plugin.layers import Linear, linear_relu_ln
    g = torch.Generator().manual_seed(5)
    seq = nn.Sequential(*linear_relu_ln(D, 1, 2), Linear(D, 10))
    norm = nn.LayerNorm(D)
    with torch.no_grad():
        for p in list(seq.parameters()) + list(norm.parameters()):
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.5) + (1.0 if p.dim() == 1 else 0.0))
    x = (torch.randn(n, D, generator=g) * 3 + 0.7).cuda()
    x2 = torch.randn(n, D, generator=g).cuda()
    return seq.cuda(), norm.cuda(), x, x2


@pytest.mark.parametrize("form,n", [("rows4", 5), ("rows32", 33)])
@pytest.mark.parametrize("live", [None, 3, 0])
def test_layernorm_only_job_equals_the_full_launch(monkeypatch, form, n, live):
    from simpb_amd.plugin import fused
    monkeypatch.setattr(fused, "WIDE_ROWS", 1 if form == "rows32" else 1 << 30)
    seq, norm, x, x2 = _chain_operands(n)
    ml = torch.tensor([live], dtype=torch.int32, device="cuda") if live is not None else None
    ln_full = torch.full((n + 2, D), SENT, device="cuda")
    ln_only = torch.full((n + 2, D), SENT, device="cuda")
    out = torch.full((n, 10), SENT, device="cuda")
    fused.run_chains([dict(plan=fused.plan_of(seq), x=(x, D, 0), x2=(x2, D, 0), out=(out, 10, 0), ln=(norm, (ln_full, D)))],
                     n, x.device, m_live=ml)
    fused.run_chains([dict(plan=None, x=(x, D, 0), ln=(norm, (ln_only, D)))], n, x.device, m_live=ml)
    torch.cuda.synchronize()
    what = (form, n, live)
    assert not bool((out == SENT).any()), what                     # (the full launch did run its chain)
    assert torch.equal(ln_only.view(torch.int32), ln_full.view(torch.int32)), (what, "ln_out differs from the full launch's")
    assert bool((ln_only[n:] == SENT).all()), (what, "rows past num_rows written")
    cut = n if live is None else live
    assert bool((ln_only[cut:n] == 0).all()), (what, "rows at and past m_live are not zeros")
    if cut:
        want = torch.nn.functional.layer_norm(x[:cut].double(), (D,), norm.weight.detach().double(), norm.bias.detach().double(), 1e-5)
        # fp32 LayerNorm of 256 values of magnitude <= ~15: a few ulp of the largest term (2^-23 * 16 * a small count)
        assert float((ln_only[:cut].double() - want).abs().max()) <= 2e-5, what


def test_a_job_without_out_must_be_the_layernorm_stage_alone():
    from simpb_amd.plugin import fused
    seq, norm, x, x2 = _chain_operands(5)
    with pytest.raises(ValueError):   # no ln_out: nothing would be written
        fused.run_chains([dict(plan=None, x=(x, D, 0), ln=(norm, None))], 5, x.device)
    with pytest.raises(ValueError):   # no leading LayerNorm at all
        fused.run_chains([dict(plan=None, x=(x, D, 0))], 5, x.device)
