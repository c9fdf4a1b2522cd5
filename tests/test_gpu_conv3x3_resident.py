"""The resident 3x3 form of csrc/conv3x3.hip (variants 12 and 13: the TH x 16 tile of input pixels with its halo stays in LDS,
the nine taps are addresses into it) against the float64 statement of tests/conv_ref.py, with the operands, the bound (e)
with its KAPPA, the one-hot rule (x) and the sentinel-guarded buffers of tests/test_backbone_float64.py (imported, not
copied).

Maps straddle the 2-D tile: one pixel, a row one short of and one past the tile's width, one past the tile both ways, the
odd (3, 5, 7), exactly one tile, and two images of two tiles each (a tile edge on an image edge: the halo of one image
must not read the next). Cin 64, 128 and 256 (all the form takes); Cout 8, 72 (a ragged last channel tile), 64 and 136
(two 64-channel tiles or a ragged second 128-channel tile). Every case is launched twice: the same bits. And every case
gives the bits of the staged form it replaces under variant 0 (7 below 128 output channels, 8 from there): the resident
form adds the same matrix instructions in the same order, so choosing it changes nothing a frame computes. Stride 2 is not
built: tests/test_conv3x3_resident_rule.py holds its refusal."""
import pytest
import torch

from tests import conv_ref as R  # noqa: F401  (the float64 statement behind case3 / judge)
from tests.test_backbone_float64 import (PYRAMID, TOK_BS, TOK_CAMS, TOK_MAP, Tally, case3, dev3, guard, judge, judge_tokens,  # noqa: F401
                                         layout_problems, nhwc_cpu, out_hw, token_buffers, with_relu)

gpu = pytest.mark.gpu

TW = 16
TH = {12: 4, 13: 8}          # rows of output pixels per workgroup (x 16 columns)
BN = {12: 64, 13: 128}       # output channels per workgroup
CINS, COUTS = (64, 128, 256), (8, 72, 64, 136)
KINDS = ("randn", "cancel", "onehot0", "onehot1")


def maps_of(variant):
    th = TH[variant]
    return [(1, 1, 1), (1, 1, TW - 1), (1, 1, TW + 1), (1, th + 1, TW + 1), (3, 5, 7), (1, th, TW), (2, th, 2 * TW)]


def staged_of(cout):
    return 7 if cout < 128 else 8


@gpu
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("variant", sorted(TH))
def test_conv3x3_resident_vs_float64_and_staged_bits(variant, cin, guard):
    from simpb_amd.plugin.ops import conv3x3_nhwc
    t = Tally(f"conv3x3 v{variant} (resident {TH[variant]} x {TW} px x {BN[variant]} ch) cin {cin}")
    for cout in COUTS:
        for m in maps_of(variant):
            for kind in KINDS:
                key = (m, 1, (cin, cout), kind)
                c = case3(*key)
                x, w, b = dev3(key)
                ho, wo = out_hw(m[1], m[2], 1)
                for relu in (False, True):
                    where = (m, cout, kind, relu)
                    y = conv3x3_nhwc(x, w, b, relu=relu, stride=1, variant=variant)
                    for p in guard.problems(y) + layout_problems(y, (m[0], cout, ho, wo)):
                        t.fail(where, p)
                    again = conv3x3_nhwc(x, w, b, relu=relu, stride=1, variant=variant)
                    for p in guard.problems(again):
                        t.fail(where, "second launch:", p)
                    if not torch.equal(y.view(torch.int16), again.view(torch.int16)):
                        t.fail(where, "two launches differ")
                    judge(t, where, nhwc_cpu(y), with_relu(c["pre"], relu), kind, "map")
                    old = conv3x3_nhwc(x, w, b, relu=relu, stride=1, variant=staged_of(cout))
                    guard.problems(old)
                    if not torch.equal(y.view(torch.int16), old.view(torch.int16)):
                        t.fail(where, f"not the bits of variant {staged_of(cout)}")
    t.finish()


@gpu
@pytest.mark.parametrize("f32", [True, False], ids=["f32_and_f16", "f16_alone"])
@pytest.mark.parametrize("variant", sorted(TH))
def test_conv3x3_resident_token_rows(variant, f32):
    from simpb_amd.plugin.ops import conv3x3_nhwc
    t = Tally(f"conv3x3 tokens v{variant} {'f32+f16' if f32 else 'f16'}")
    per_cam, start = 3 * 5 + 9, 4           # level_start > 0, tokens_per_cam larger than the level
    for cp in ((64, 72), (128, 64), (256, 136)):
        for kind in ("randn", "onehot0", "onehot1"):
            key = (TOK_MAP, 1, cp, kind)
            c = case3(*key)
            x, w, b = dev3(key)
            bits = []
            for v in (variant, variant, staged_of(cp[1])):
                t32, t16, wholes = token_buffers(TOK_BS, TOK_CAMS * per_cam, cp[1], f32)
                out = conv3x3_nhwc(x, w, b, relu=False, stride=1, tokens=(t32, per_cam, start, t16), variant=v)
                if out is not None:
                    t.fail(cp, kind, "token form returned a tensor")
                judge_tokens(t, (cp, kind, v), t32, t16, wholes, [c["pre"]], [start], per_cam, kind)
                bits.append((t16.view(torch.int16).cpu(), None if t32 is None else t32.view(torch.int32).cpu()))
            if not torch.equal(bits[0][0], bits[1][0]):
                t.fail(cp, kind, "two launches differ")
            if not torch.equal(bits[0][0], bits[2][0]) or (f32 and not torch.equal(bits[0][1], bits[2][1])):
                t.fail(cp, kind, f"not the rows of variant {staged_of(cp[1])}")
    t.finish()


@gpu
@pytest.mark.parametrize("f32", [True, False], ids=["f32_and_f16", "f16_alone"])
@pytest.mark.parametrize("cp", [(256, 256), (64, 72)], ids=["256to256", "64to72"])
def test_conv3x3_group_resident_levels_give_the_staged_rows(cp, f32):
    """The group launch on PYRAMID with every level resident, with the forms mixed (two launches) and as the library's own
    rule has it: the float64 bound, and the rows of the launch with the staged form forced for every level, bit for bit."""
    from simpb_amd.plugin.ops import conv3x3_group_tokens
    t = Tally(f"conv3x3 group, resident levels, {cp[0]}->{cp[1]} {'f32+f16' if f32 else 'f16'}")
    starts, at = [], 3                      # level_start > 0, a gap of two rows between levels, five spare rows behind
    for h, w in PYRAMID:
        starts.append(at)
        at += h * w + 2
    per_cam = at + 5
    n = TOK_BS * TOK_CAMS
    for kind in ("randn", "onehot0", "onehot1"):
        keys = [((n, h, w), 1, cp, kind) for h, w in PYRAMID]
        cs = [case3(*k) for k in keys]
        ds = [dev3(k) for k in keys]
        rows = {}
        for forms in ((8, 8, 8, 8), (13, 13, 13, 13), (13, 8, 13, 8), None):
            t32, t16, wholes = token_buffers(TOK_BS, TOK_CAMS * per_cam, cp[1], f32)
            conv3x3_group_tokens([d[0] for d in ds], [d[1] for d in ds], [d[2] for d in ds], t32, per_cam, starts, col16=t16, variants=forms)
            judge_tokens(t, (kind, forms), t32, t16, wholes, [c["pre"] for c in cs], starts, per_cam, kind)
            rows[forms] = (t16.view(torch.int16).cpu(), None if t32 is None else t32.view(torch.int32).cpu())
        for forms, got in rows.items():
            if not torch.equal(got[0], rows[(8, 8, 8, 8)][0]) or (f32 and not torch.equal(got[1], rows[(8, 8, 8, 8)][1])):
                t.fail(kind, forms, "not the rows of the staged group launch")
    t.finish()
