"""The second selection rule of csrc/conv3x3.hip (no GPU): simpb_conv3x3_choose_resident, which variant 0 asks after the tile
rule has answered 7 or 8, and simpb_conv3x3_group_choose_resident, which the FPN's group launch asks once. Restated here;
yes only where the tile rule says 7 or 8; on the real ResNet50 / FPN launches at 6 x 256 x 704 what
profiles/conv3x3_large_maps.md records as measured; and the refusals of a forced resident variant."""
import ctypes

import pytest

from tests.test_backbone_float64 import chosen3

# (images, H, W, Cin, Cout) -> what the profile note measured as the fastest form that is faster than the staged one
MEASURED = {(6, 64, 176, 64, 64): 12, (6, 32, 88, 128, 128): 12, (6, 64, 176, 256, 256): 13, (6, 32, 88, 256, 256): 12}
PYRAMID_REAL = [(64, 176), (32, 88), (16, 44), (8, 22)]
EINVAL = 1


def resident_restated(n, h, w, cin, cout, stride):
    if stride != 1 or cin not in (64, 128, 256) or cout != cin:
        return 0
    if chosen3(n * h * w, cout) not in (7, 8):
        return 0
    across = -(-w // 16)
    t13 = n * -(-h // 8) * across * -(-cout // 128)
    t12 = n * -(-h // 4) * across * -(-cout // 64)
    if cin == 256 and t13 >= 1024:
        return 13
    return 12 if t12 >= 512 else 0


def test_resident_rule_is_the_restated_one_and_only_where_the_tile_rule_says_7_or_8():
    from simpb_amd.plugin.ops import conv3x3_resident_for, conv3x3_variant_for
    yes = 0
    for n in (1, 6):
        for h, w in ((1, 1), (8, 16), (8, 22), (16, 44), (32, 88), (33, 89), (64, 176), (96, 128), (128, 352), (256, 704)):
            for cin in (64, 128, 192, 256, 320, 512):
                for cout in (8, 64, 72, 128, 136, 256, 512):
                    for stride in (1, 2):
                        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
                        got = conv3x3_resident_for(n * ho * wo, h, w, cin, cout, stride)
                        assert got == resident_restated(n, h, w, cin, cout, stride), (n, h, w, cin, cout, stride, got)
                        if got:
                            yes += 1
                            assert stride == 1 and conv3x3_variant_for(n * h * w, cin, cout) in (7, 8), (n, h, w, cin, cout)
    assert yes > 0


def test_resident_rule_on_the_real_launches():
    from simpb_amd.plugin.ops import conv3x3_group_resident_for, conv3x3_resident_for
    for (n, h, w, cin, cout), want in MEASURED.items():
        assert conv3x3_resident_for(n * h * w, h, w, cin, cout, 1) == want, (n, h, w, cin, cout)
    # stride 2 (layer2.0 conv2) and the small maps keep their forms
    assert conv3x3_resident_for(6 * 32 * 88, 64, 176, 128, 128, 2) == 0
    assert conv3x3_resident_for(6 * 16 * 44, 16, 44, 256, 256, 1) == 0
    assert conv3x3_resident_for(6 * 8 * 22, 8, 22, 512, 512, 1) == 0
    # the FPN's group launch: every level resident on the real pyramid; the staged launch on small ones and other channels
    assert conv3x3_group_resident_for(6, PYRAMID_REAL, 256, 256) == 13
    assert conv3x3_group_resident_for(6, [(4, 11), (2, 6), (1, 3), (1, 1)], 256, 256) == 0
    assert conv3x3_group_resident_for(6, PYRAMID_REAL, 64, 72) == 0


@pytest.mark.parametrize("variant", (12, 13))
def test_forced_resident_variant_refuses_what_it_does_not_take(variant):
    """Cin that is not resident-sized, stride 2 (not built) and Cin % 64 != 0 return SIMPB_EINVAL before anything is
    launched (the pointers are never read: validation comes first)."""
    from simpb_amd import _lib
    fn = _lib.lib().simpb_conv3x3_nhwc_f16
    p = ctypes.c_void_p(4096)

    def call(cin, cout, stride, v):
        return fn(p, None, None, 0, 0, p, p, p, 1, 8, 16, cin, cout, stride, 1, v, None)

    assert call(192, 64, 1, variant) == EINVAL     # a multiple of 64 that is not 64, 128 or 256
    assert call(320, 64, 1, variant) == EINVAL
    assert call(512, 64, 1, variant) == EINVAL
    assert call(64, 64, 2, variant) == EINVAL      # stride 2
    assert call(256, 256, 2, variant) == EINVAL
    assert call(96, 64, 1, variant) == EINVAL      # Cin % 64 != 0
    assert call(64, 64, 1, 14) == EINVAL           # past the last variant
