"""The 64 x 64 staged tilings of csrc/conv3x3.hip that split K over groups of waves inside the workgroup (variants 9-11:
conv_staged_ksplit_kernel with 1, 2 and 4 groups) and the pointwise 64 x 64 tiling (conv1x1 variant 4) against the float64
statement of tests/conv_ref.py, with the operands, the bound (e) with its KAPPA, the one-hot rule (x) and the
sentinel-guarded buffers of tests/test_backbone_float64.py (imported, not copied).

Maps straddle the 64-pixel tile: one pixel, 63, 65, the odd (3, 5, 7) and exactly two tiles, each at stride 1 and 2.
Channel pairs put the K split on its edges: Cin 64 = 9 chunks (with 4 groups the last step has a chunk for one group only,
with 2 groups for one of two), 128 = 18 chunks (4 groups: the last step has two chunks), 320 = 45 chunks (an uneven share
at 2 and at 4 groups); Cout 8, 72 (a ragged last channel tile) and 64. Every case is launched twice: the two results are
the same bits. Variants 9 and 11 and conv1x1 variant 4 are what variant 0 runs where it ran 1, 4 and 2: they must give
those forms' outputs bit for bit. The host test (no GPU) holds variant 0's choice to the rule of before outside the region
the new forms were measured for."""
import pytest
import torch

from tests import conv_ref as R  # noqa: F401  (the float64 statement behind case3 / case1 / judge)
from tests.test_backbone_float64 import (CPAIRS3, SELECT3, TOK_BS, TOK_CAMS, TOK_MAP, Tally, case1, case3, cases3, chosen3, dev1, dev3,
                                         guard, judge, judge_tokens, layout_problems, nhwc_cpu, out_hw, token_buffers, with_relu)  # noqa: F401

gpu = pytest.mark.gpu

TILE = {9: 64, 10: 64, 11: 64}            # output pixels per workgroup (x 64 channels)
WAVES = {9: 4, 10: 8, 11: 16}
CINS, COUTS = (64, 128, 320), (8, 72, 64)
KINDS = ("randn", "cancel", "onehot0", "onehot1")
# the 3x3 launches of ResNet50 + FPN at 6 x 256 x 704: (output pixels, Cin, Cout)
REAL3 = [(67584, 64, 64), (16896, 128, 128), (16896, 128, 128), (4224, 256, 256), (4224, 256, 256), (1056, 512, 512), (1056, 512, 512),
         (67584, 256, 256), (16896, 256, 256), (4224, 256, 256), (1056, 256, 256)]
# what variant 0 runs in the measured region (Cin >= 256 where the rule of before chose 1 or 4): profiles/conv3x3_small_maps.md
MEASURED = {(4224, 256, 256): 9, (1056, 512, 512): 11}


def maps_of(variant):
    t = TILE[variant]
    return [(1, 1, 1), (1, 1, t - 1), (1, 1, t + 1), (3, 5, 7), (1, 2, t)]


@gpu
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("variant", sorted(TILE))
def test_conv3x3_ksplit_vs_float64(variant, cin, guard):
    from simpb_amd.plugin.ops import conv3x3_nhwc
    t = Tally(f"conv3x3 v{variant} ({TILE[variant]} px, {WAVES[variant]} waves) cin {cin}")
    for cout in COUTS:
        for m in maps_of(variant):
            for stride in (1, 2):
                for kind in KINDS:
                    key = (m, stride, (cin, cout), kind)
                    c = case3(*key)
                    x, w, b = dev3(key)
                    ho, wo = out_hw(m[1], m[2], stride)
                    for relu in (False, True):
                        where = (m, stride, cout, kind, relu)
                        y = conv3x3_nhwc(x, w, b, relu=relu, stride=stride, variant=variant)
                        for p in guard.problems(y) + layout_problems(y, (m[0], cout, ho, wo)):
                            t.fail(where, p)
                        again = conv3x3_nhwc(x, w, b, relu=relu, stride=stride, variant=variant)
                        for p in guard.problems(again):
                            t.fail(where, "second launch:", p)
                        if not torch.equal(y.view(torch.int16), again.view(torch.int16)):
                            t.fail(where, "two launches differ")
                        judge(t, where, nhwc_cpu(y), with_relu(c["pre"], relu), kind, "map")
    t.finish()


@gpu
@pytest.mark.parametrize("f32", [True, False], ids=["f32_and_f16", "f16_alone"])
@pytest.mark.parametrize("variant", sorted(TILE))
def test_conv3x3_ksplit_token_rows_vs_float64(variant, f32):
    from simpb_amd.plugin.ops import conv3x3_nhwc
    t = Tally(f"conv3x3 tokens v{variant} {'f32+f16' if f32 else 'f16'}")
    per_cam, start = 3 * 5 + 9, 4           # level_start > 0, tokens_per_cam larger than the level
    for cp in ((64, 72), (128, 64)):
        for kind in ("randn", "onehot0", "onehot1"):
            key = (TOK_MAP, 1, cp, kind)
            c = case3(*key)
            x, w, b = dev3(key)
            bits = []
            for _ in range(2):
                t32, t16, wholes = token_buffers(TOK_BS, TOK_CAMS * per_cam, cp[1], f32)
                out = conv3x3_nhwc(x, w, b, relu=False, stride=1, tokens=(t32, per_cam, start, t16), variant=variant)
                if out is not None:
                    t.fail(cp, kind, "token form returned a tensor")
                judge_tokens(t, (cp, kind), t32, t16, wholes, [c["pre"]], [start], per_cam, kind)
                bits.append(t16.view(torch.int16).cpu())
            if not torch.equal(bits[0], bits[1]):
                t.fail(cp, kind, "two launches differ")
    t.finish()


@gpu
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("new,old", [(9, 1), (11, 4)])
def test_conv3x3_staged_forms_give_the_direct_forms_bits(new, old, stride):
    """Variant 0 runs 9 where it ran 1 and 11 where it ran 4. Both add the chunks of a tile in the order of the form they
    replace, with the same eight k-values in every matrix instruction: every output is the same f16, so the choice of variant 0
    changes nothing a frame computes. Maps with ragged tiles of both forms, a ragged channel tile, uneven K shares."""
    from simpb_amd.plugin.ops import conv3x3_nhwc
    for m, cp in (((3, 5, 7), (64, 72)), ((1, 2, 64), (128, 64)), ((2, 9, 13), (320, 72)), ((6, 8, 22), (512, 128))):
        for kind in ("randn", "cancel"):
            x, w, b = dev3((m, stride, cp, kind))
            for relu in (False, True):
                y_new = conv3x3_nhwc(x, w, b, relu=relu, stride=stride, variant=new)
                y_old = conv3x3_nhwc(x, w, b, relu=relu, stride=stride, variant=old)
                assert torch.equal(y_new.view(torch.int16), y_old.view(torch.int16)), (new, old, m, stride, cp, kind, relu)


@gpu
def test_conv1x1_64x64_tiling_gives_the_128x64_tilings_bits():
    """conv1x1 variant 4 is what variant 0 runs for Cin >= 1024 on the small maps, where it ran 2: the same pipeline at
    another tile, the same chunks in the same order -- the same f16 outputs."""
    from simpb_amd.plugin.ops import conv1x1_nhwc
    for m, stride, cin, cout, form in (((1, 8, 16), 1, 1024, 72, "res"), ((1, 1, 65), 2, 2048, 64, "plain"), ((6, 8, 22), 1, 2048, 256, "plain")):
        x, w, b, res, _ = dev1((m, stride, cin, cout, "randn", form))
        for relu in (False, True):
            y4 = conv1x1_nhwc(x, w, b, residual=res, relu=relu, stride=stride, variant=4)
            y2 = conv1x1_nhwc(x, w, b, residual=res, relu=relu, stride=stride, variant=2)
            assert torch.equal(y4.view(torch.int16), y2.view(torch.int16)), (m, stride, cin, cout, form, relu)


@gpu
@pytest.mark.parametrize("cin", (1024, 2048))
@pytest.mark.parametrize("variant", (4,))
def test_conv1x1_64x64_tiling_vs_float64(variant, cin, guard):
    from simpb_amd.plugin.ops import conv1x1_nhwc
    t = Tally(f"conv1x1 v{variant} (64 x 64) cin {cin}")
    for cout in (64, 72):
        for m in ((1, 1, 63), (1, 1, 65), (1, 8, 16)):
            for stride in (1, 2):
                for kind, form in (("randn", "plain"), ("randn", "res"), ("onehot0", "plain"), ("onehot0", "res")):
                    key = (m, stride, cin, cout, kind, form)
                    c = case1(*key)
                    x, w, b, res, _ = dev1(key)
                    ho, wo = out_hw(m[1], m[2], stride)
                    for relu in (False, True):
                        where = (m, stride, cout, kind, form, relu)
                        y = conv1x1_nhwc(x, w, b, residual=res, relu=relu, stride=stride, variant=variant)
                        for p in guard.problems(y) + layout_problems(y, (m[0], cout, ho, wo)):
                            t.fail(where, p)
                        again = conv1x1_nhwc(x, w, b, residual=res, relu=relu, stride=stride, variant=variant)
                        guard.problems(again)
                        if not torch.equal(y.view(torch.int16), again.view(torch.int16)):
                            t.fail(where, "two launches differ")
                        judge(t, where, nhwc_cpu(y), with_relu(c["pre"], relu), kind, form)
    t.finish()


def test_variant0_keeps_the_rule_outside_the_measured_region():
    """simpb_conv3x3_choose_variant (what variant 0 launches) on every (output pixels, Cin, Cout) that
    tests/test_backbone_float64.py runs under variant 0 and on the real ResNet50 / FPN launches: outside Cin >= 256 with the
    rule of before choosing 1 or 4 it is that rule; inside, the rule's choice or one of the new forms, and on the real shapes
    what profiles/conv3x3_small_maps.md measured as the fastest."""
    from simpb_amd.plugin.ops import conv3x3_variant_for
    shapes = {(m[0] * out_hw(m[1], m[2], stride)[0] * out_hw(m[1], m[2], stride)[1], cp[0], cp[1]) for m, stride, cp, _ in cases3(0)}
    shapes |= {(m[0] * m[1] * m[2], cp[0], cp[1]) for m, cp, _ in SELECT3} | set(REAL3)
    shapes |= {(p, cin, cout) for cin in (64, 192, 256, 320, 512) for cout in (8, 64, 72, 256, 512)
               for p in (1, 63, 1056, 2048, 2049, 4224, 8192, 8193, 16896, 24576, 67584, 300000)}
    assert {cp for _, cp0, cp1 in shapes for cp in [(cp0, cp1)]} >= set(CPAIRS3)
    for p_out, cin, cout in sorted(shapes):
        before, now = chosen3(p_out, cout), conv3x3_variant_for(p_out, cin, cout)
        inside = cin >= 256 and before in (1, 4)
        print(f"FIG variant 0: {p_out} px {cin}->{cout}: {now}" + ("" if now == before else f" (before: {before})"))
        if not inside:
            assert now == before, (p_out, cin, cout, now, before)
        else:
            assert now == before or now in TILE, (p_out, cin, cout, now, before)
    for shape, want in MEASURED.items():
        assert conv3x3_variant_for(*shape) == want, (shape, want)
    for m, cp, expect in SELECT3:           # the selection edges that module asserts, through the exported function
        assert conv3x3_variant_for(m[0] * m[1] * m[2], *cp) == expect
