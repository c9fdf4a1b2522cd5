"""CPU: the host side of camera dropout -- the argument validation of the six `_cams` entry points (it runs before any
HIP call), the runners' mask normalisation (runner.normalise_cameras) with its refusals, and the subset-oracle recipe of
tests/camera_dropout_ref.py as a self-check of the yardstick the GPU tests use."""
import ctypes

import pytest
import torch

from simpb_amd import _lib, build, synth
from simpb_amd.runner import normalise_cameras
from tests import camera_dropout_ref as C
from tests.helpers import build_product_head, load_golden, spec_of


def test_cams_entry_points_validate_before_any_hip_call():
    """As tests/test_capi.py::test_bad_arguments_return_einval: no device in the process."""
    build.build_extension()
    h = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)
    P = lambda n, v: [v] * n   # noqa: E731
    f5 = (704.0, 256.0, 35.0, 35.0, 10.0)
    # simpb_alloc_project_cams: 5 pointers, bs, A, cams, 5 floats, cam_valid, stream
    assert h.simpb_alloc_project_cams(*P(5, null), 3, 48, 6, *f5, one, null) == 1
    assert h.simpb_alloc_project_cams(*P(5, null), 3, 48, 6, *f5, null, null) == 1
    assert h.simpb_alloc_project_cams(*P(5, one), 3, 48, 0, *f5, one, null) == 1
    assert h.simpb_alloc_project_cams(*P(5, one), 0, 48, 6, *f5, one, null) == 1
    # simpb_alloc_static_cams: 15 pointers, bs, A, cams, capacity, 5 floats, cam_valid, stream
    assert h.simpb_alloc_static_cams(*P(15, null), 3, 48, 6, 128, *f5, one, null) == 1
    assert h.simpb_alloc_static_cams(*P(15, one), 3, 48, 9, 128, *f5, one, null) == 1   # at most 8 cameras
    assert h.simpb_alloc_static_cams(*P(15, one), 3, 48, 6, 0, *f5, one, null) == 1
    # simpb_alloc_ragged_cams: 15 pointers, bs, A, cams, per_stream, 5 floats, active, cam_valid, stream
    assert h.simpb_alloc_ragged_cams(*P(15, null), 3, 48, 6, 128, *f5, one, one, null) == 1
    assert h.simpb_alloc_ragged_cams(*P(15, null), 3, 48, 6, 128, *f5, null, null, null) == 1
    assert h.simpb_alloc_ragged_cams(*P(15, one), 17, 48, 6, 128, *f5, null, one, null) == 1   # 102 groups
    assert h.simpb_alloc_ragged_cams(*P(15, one), 3, 48, 6, 0, *f5, one, one, null) == 1
    # simpb_dfa_points_cams: 7 pointers, bs, A, num_fix, num_learn, cams, cam_valid, stream
    assert h.simpb_dfa_points_cams(*P(7, null), 2, 77, 7, 6, 6, one, null) == 1
    assert h.simpb_dfa_points_cams(*P(7, one), 2, 77, 0, 0, 6, one, null) == 1
    assert h.simpb_dfa_points_cams(one, null, one, null, one, one, one, 2, 77, 7, 6, 6, one, null) == 1   # learnable missing
    # simpb_dfa_weights_cams: 3 pointers, bs, A, cams, levels, pts, groups, cam_valid, stream
    assert h.simpb_dfa_weights_cams(*P(3, null), 2, 77, 6, 4, 13, 8, one, null) == 1
    assert h.simpb_dfa_weights_cams(*P(3, one), 2, 77, 6, 4, 13, 512, one, null) == 1
    assert h.simpb_dfa_weights_cams(*P(3, one), 2, 77, 60, 4, 13, 8, one, null) == 1   # the softmax row does not fit LDS
    # simpb_dfa_fused_forward_cams: out, feat, is_f16, 11 pointers, bs, cams, num_feat, C, L, A, num_fix, num_learn, G,
    # cam_valid, stream
    shipped = (2, 6, 1000, 256, 4, 77, 7, 6, 8)
    assert h.simpb_dfa_fused_forward_cams(null, null, 0, *P(11, null), *shipped, one, null) == 1
    assert h.simpb_dfa_fused_forward_cams(one, one, 0, *P(11, one), 2, 5, 1000, 256, 4, 77, 7, 6, 8, one, null) == 1   # shipped layout only
    assert h.simpb_dfa_fused_forward_cams(one, one, 1, *P(11, one), 0, 6, 1000, 256, 4, 77, 7, 6, 8, one, null) == 1
    assert h.simpb_abi_version() == 7


def test_mask_normalisation():
    full = [[True] * 6] * 2
    assert normalise_cameras(None, 2, 6) is None
    assert normalise_cameras(full, 2, 6) is None                      # all true: today's path
    assert normalise_cameras([[1, 0, 1, 1, 1, 1], [1] * 6], 2, 6) == ((True, False, True, True, True, True), (True,) * 6)
    assert normalise_cameras([[0] * 5 + [1]], 1, 6) == ((False,) * 5 + (True,),)
    # active=False overrides the stream's row: it is not looked at, and a full rig beside it is today's path
    assert normalise_cameras([[1] * 6, [0] * 6], 2, 6, active=[True, False]) is None
    assert normalise_cameras([[1, 1, 0, 1, 1, 1], [0, 1, 0, 1, 0, 1]], 2, 6, active=[True, False]) == (
        (True, True, False, True, True, True), (True,) * 6)


def test_masks_that_cannot_be_honoured_are_refused():
    with pytest.raises(ValueError):   # one row for two streams
        normalise_cameras([[1] * 6], 2, 6)
    with pytest.raises(ValueError):   # five entries for six cameras
        normalise_cameras([[1] * 6, [1] * 5], 2, 6)
    with pytest.raises(ValueError):   # a stream without any frame is paused, not masked
        normalise_cameras([[1] * 6, [0] * 6], 2, 6)
    with pytest.raises(ValueError):
        normalise_cameras([[1] * 6, [0] * 6], 2, 6, active=[False, True])
    with pytest.raises(ValueError):   # the activity mask has its own length check
        normalise_cameras([[1] * 6, [1] * 6], 2, 6, active=[True])


def test_subset_oracle_with_all_six_cameras_is_the_oracle(monkeypatch):
    """Frame 0 through the recipe with kept = all six equals the unpatched oracle bit for bit; with a camera dropped the
    oracle runs unchanged and its 2D set loses exactly that camera's group."""
    from oracle import simpb_ref as R
    spec = spec_of(load_golden("head_small.npz"))
    head = build_product_head(spec, "cpu")
    synth.load_procedural(head, seed=5)
    params = {k: v.detach() for k, v in head.state_dict().items()}
    make = lambda: R.OracleHead(params, head.operation_order, spec["num_anchor"], spec["num_temp"], spec["num_output"])  # noqa: E731
    maps = synth.feature_maps_nchw(spec["bs"], 0, spec["image_wh"], seed=9)
    metas = synth.frame_metas(spec["bs"], 0, spec["image_wh"])
    with torch.no_grad():
        plain = make().forward(R.feature_maps_format(maps), metas)
        want, cuts = C.oracle_frame(monkeypatch, make(), maps, metas, C.ALL)
        less, _ = C.oracle_frame(monkeypatch, make(), maps, metas, (0, 2, 3, 4, 5))
    assert cuts["update"] is None and cuts["cache"] >= 0.0
    for k in ("prediction", "classification", "quality", "prediction2d", "classification2d"):
        for a, b in zip(want[k], plain[k]):
            assert (a is None and b is None) or torch.equal(a, b), k
    assert torch.equal(want["instance_id"], plain["instance_id"])
    groups, fewer = plain["ref_query_groups_list"][0], less["ref_query_groups_list"][0]
    assert len(groups) == 6 and len(fewer) == 5
    sizes = [hi - lo for lo, hi in groups]
    assert [hi - lo for lo, hi in fewer] == sizes[:1] + sizes[2:] and sizes[1] > 0   # the first layer starts from the learned anchors
    # dropping a camera is no small change: already on the cold frame an order of magnitude above the GPU tests' 1e-3
    assert float((less["prediction"][-1] - plain["prediction"][-1]).abs().max()) > 1e-2


def test_decode_static_host_gives_a_masked_camera_an_empty_2d_list():
    """The 2D record of a frame without camera 1: no slot carries that camera, so its group is empty and no 2D box is listed
    for it; the other cameras' boxes and their association are as ever."""
    import numpy as np
    from simpb_amd.plugin.detection3d import SparseBox3DDecoder
    rec3d = np.zeros((1, 4, 15), np.float32)
    cams = [0, 0, 2, 3, 3, 5]
    rec2d = np.zeros((1, 8, 8), np.float32)
    rec2d[0, :, 6:] = -1                       # capacity slots: rank -1, camera -1
    for s, c in enumerate(cams):
        rec2d[0, s] = [10 * s, 1, 10 * s + 5, 6, 0.5, 2, s % 4, c]
    out = SparseBox3DDecoder.decode_static_host(rec3d, rec2d, 6)[0]
    assert out["camidx_2d"].tolist() == [float(c) for c in cams] and len(out["boxes_2d"]) == 6
    groups = out["query_groups"]
    assert groups[1][0] == groups[1][1] and [hi - lo for lo, hi in groups] == [2, 0, 1, 2, 0, 1]
    assert tuple(out["trans_matrix"].shape) == (4, 6) and float(out["trans_matrix"].sum()) == 6.0
