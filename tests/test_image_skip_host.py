"""Skipping the backbone's work on idle images, the host side (no GPU): runner.live_images, the four *_live entry points
(declared in include/simpb_hip.h, exported by the library, refusing what the entry points without the suffix refuse before
anything is launched) and the runners' `idle_images` keyword."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE_ENTRIES = ("simpb_stem_conv7x7_pool_f16_live", "simpb_conv1x1_nhwc_f16_live", "simpb_conv3x3_nhwc_f16_live",
                "simpb_conv3x3_group_tokens_forms_f16_live")
EINVAL = 1


def check_table(table, bs, cams, want):
    assert isinstance(table, np.ndarray) and table.dtype == np.int32 and table.shape == (1 + bs * cams,)
    n = int(table[0])
    assert n == len(want)
    assert table[1:1 + n].tolist() == want
    assert all(a < b for a, b in zip(want, want[1:]))   # strictly ascending
    assert not table[1 + n:].any()


def test_live_images_of_a_full_frame():
    from simpb_amd.runner import live_images
    check_table(live_images(None, None, 2, 6), 2, 6, list(range(12)))
    check_table(live_images(None, None, 1, 1), 1, 1, [0])
    check_table(live_images((True, True), ((True,) * 3,) * 2, 2, 3), 2, 3, list(range(6)))


def test_live_images_with_pauses_only():
    from simpb_amd.runner import live_images
    check_table(live_images((True, False, True), None, 3, 2), 3, 2, [0, 1, 4, 5])
    check_table(live_images((False, False, False, True), None, 4, 6), 4, 6, list(range(18, 24)))
    check_table(live_images((False, False), None, 2, 6), 2, 6, [])


def test_live_images_with_cameras_only():
    from simpb_amd.runner import live_images
    cams = ((True, False, True), (False, True, True))
    check_table(live_images(None, cams, 2, 3), 2, 3, [0, 2, 4, 5])


def test_live_images_with_both_and_a_paused_row_ignored():
    from simpb_amd.runner import live_images, normalise_cameras
    cams = ((True, True, False), (False, False, False), (False, True, True))
    check_table(live_images((True, False, True), cams, 3, 3), 3, 3, [0, 1, 7, 8])
    # the same whatever the paused stream's row says, and through normalise_cameras (which hands it back all True)
    other = ((True, True, False), (True, True, True), (False, True, True))
    assert (live_images((True, False, True), other, 3, 3) == live_images((True, False, True), cams, 3, 3)).all()
    norm = normalise_cameras(other, 3, 3, (True, False, True))
    check_table(live_images((True, False, True), norm, 3, 3), 3, 3, [0, 1, 7, 8])


def test_live_images_refuses_masks_of_another_size():
    from simpb_amd.runner import live_images
    with pytest.raises(ValueError):
        live_images((True,), None, 2, 6)
    with pytest.raises(ValueError):
        live_images(None, ((True,) * 5,) * 2, 2, 6)


def test_live_entry_points_are_declared_and_exported():
    from simpb_amd import _lib
    header = open(os.path.join(ROOT, "include", "simpb_hip.h")).read()
    lib = _lib.lib()
    for name in LIVE_ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, f"{name} is not declared in include/simpb_hip.h"
        assert re.search(r"const\s+int\s*\*\s*live\s*$", decl.group(1).strip()), f"{name}: `const int* live` is the last argument"
        assert getattr(lib, name) is not None
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0][-1] is ctypes.c_void_p
    assert lib.simpb_abi_version() == 7   # additive: the version stays


@pytest.mark.parametrize("live", (None, 4096))
def test_conv3x3_live_refuses_what_conv3x3_refuses(live):
    """The refusals tests/test_conv3x3_resident_rule.py shows for simpb_conv3x3_nhwc_f16, with and without a table:
    validation comes first, no pointer is read and nothing is launched."""
    from simpb_amd import _lib
    old, new = _lib.lib().simpb_conv3x3_nhwc_f16, _lib.lib().simpb_conv3x3_nhwc_f16_live
    p = ctypes.c_void_p(4096)
    t = ctypes.c_void_p(live) if live else None
    for cin, cout, stride, v in ((192, 64, 1, 12), (320, 64, 1, 13), (512, 64, 1, 12), (64, 64, 2, 12), (256, 256, 2, 13),
                                 (96, 64, 1, 12), (64, 64, 1, 14), (64, 64, 3, 1), (64, 12, 1, 1), (64, 64, 1, -1)):
        assert old(p, None, None, 0, 0, p, p, p, 1, 8, 16, cin, cout, stride, 1, v, None) == EINVAL
        assert new(p, None, None, 0, 0, p, p, p, 1, 8, 16, cin, cout, stride, 1, v, None, t) == EINVAL, (cin, cout, stride, v)
    # no destination, two destinations, no images, a misaligned operand
    assert new(None, None, None, 0, 0, p, p, p, 1, 8, 16, 64, 64, 1, 1, 1, None, t) == EINVAL
    assert new(p, p, None, 176, 0, p, p, p, 1, 8, 16, 64, 64, 1, 1, 1, None, t) == EINVAL
    assert new(p, None, None, 0, 0, p, p, p, 0, 8, 16, 64, 64, 1, 1, 1, None, t) == EINVAL
    assert new(p, None, None, 0, 0, ctypes.c_void_p(4100), p, p, 1, 8, 16, 64, 64, 1, 1, 1, None, t) == EINVAL
    # token rows that do not fit a camera's block
    assert new(None, p, None, 100, 0, p, p, p, 1, 8, 16, 64, 64, 1, 0, 8, None, t) == EINVAL


@pytest.mark.parametrize("live", (None, 4096))
def test_conv1x1_stem_and_group_live_refuse_what_the_old_entry_points_refuse(live):
    from simpb_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(4096)
    t = ctypes.c_void_p(live) if live else None
    c11, c11_live = lib.simpb_conv1x1_nhwc_f16, lib.simpb_conv1x1_nhwc_f16_live
    #            y  x  w  b  res   n  h  w   cin cout s  relu up2 in_bias variant
    for args in ((p, p, p, p, None, 1, 8, 16, 96, 64, 1, 1, 0, None, 0),     # Cin % 64
                 (p, p, p, p, None, 1, 8, 16, 64, 12, 1, 1, 0, None, 0),     # Cout % 8
                 (p, p, p, p, None, 1, 8, 16, 64, 64, 3, 1, 0, None, 0),     # stride
                 (p, p, p, p, None, 1, 8, 16, 64, 64, 1, 1, 0, None, 5),     # variant
                 (p, p, p, p, None, 1, 8, 16, 64, 64, 1, 1, 0, p, 2),        # input_bias outside variant 1
                 (p, p, p, p, None, 1, 8, 16, 64, 64, 1, 1, 1, None, 0),     # upsampled residual without a residual
                 (p, p, p, p, p, 1, 7, 16, 64, 64, 1, 1, 1, None, 0),        # ... with an odd map
                 (None, p, p, p, None, 1, 8, 16, 64, 64, 1, 1, 0, None, 0),  # no output
                 (p, p, p, p, None, 0, 8, 16, 64, 64, 1, 1, 0, None, 0)):    # no images
        assert c11(*args, None) == EINVAL, args
        assert c11_live(*args, None, t) == EINVAL, args
    stem, stem_live = lib.simpb_stem_conv7x7_pool_f16, lib.simpb_stem_conv7x7_pool_f16_live
    for args in ((p, p, p, p, 1, 64, 176, 32), (None, p, p, p, 1, 64, 176, 64), (p, p, p, p, 0, 64, 176, 64),
                 (p, p, p, p, 70000, 64, 176, 64), (p, p, p, p, 1, 0, 176, 64), (ctypes.c_void_p(4104), p, p, p, 1, 64, 176, 64)):
        assert stem(*args, None) == EINVAL, args
        assert stem_live(*args, None, t) == EINVAL, args
    group, group_live = lib.simpb_conv3x3_group_tokens_forms_f16, lib.simpb_conv3x3_group_tokens_forms_f16_live
    ints, ptrs = ctypes.c_int * 2, ctypes.c_void_p * 2
    x, hs, ws, st = ptrs(4096, 4096), ints(8, 4), ints(22, 11), ints(0, 176)

    def call(fn, tail, levels=2, tokens=p, per_cam=220, cin=256, cout=256, variant=None, starts=st, xs=x):
        return fn(levels, tokens, None, per_cam, starts, xs, xs, xs, 1, hs, ws, cin, cout, 0, variant, None, *tail)

    for fn, tail in ((group, ()), (group_live, (t,))):
        assert call(fn, tail, levels=0) == EINVAL
        assert call(fn, tail, levels=5) == EINVAL
        assert call(fn, tail, tokens=None) == EINVAL
        assert call(fn, tail, per_cam=219) == EINVAL                 # the second level's rows do not fit
        assert call(fn, tail, cin=96) == EINVAL
        assert call(fn, tail, variant=ints(8, 7)) == EINVAL          # a form the group launch does not have
        assert call(fn, tail, cin=512, cout=512, variant=ints(13, 13)) == EINVAL   # resident form, Cin not resident-sized
        assert call(fn, tail, xs=ptrs(4096, 0)) == EINVAL


def test_idle_images_keyword():
    """Every runner takes idle_images, "compute" by default; anything else is refused before the model is looked at."""
    import inspect
    from simpb_amd import runner
    assert inspect.signature(runner.FrameRunner.__init__).parameters["idle_images"].default == "compute"
    assert runner.IDLE_IMAGES == ("compute", "skip")
    from simpb_amd.plugin import detector
    strict = detector.STRICT_NO_VENDOR   # (a pipelined runner's constructor sets it for the process)
    try:
        for cls in (runner.FrameRunner, runner.PipelinedRunner, runner.SplitPipelinedRunner):
            with pytest.raises(ValueError, match="idle_images"):
                cls(None, 2, (128, 352), idle_images="drop")
    finally:
        detector.STRICT_NO_VENDOR = strict
