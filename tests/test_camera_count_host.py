"""CPU: the host side of rigs of one to eight cameras -- the argument validation of simpb_dfa_fused_forward_rig (it runs before
any HIP call), the config / weights / refusals of a head at N cameras, simpb_amd.synth at N cameras, and the reference alone
on the inputs the GPU tests use (tests/test_gpu_camera_count_*.py): the conditions those tests rely on hold on the oracle's
own numbers, so a miss on the GPU is a miss of the product. Each test prints its figures (`FIG ...`) before it asserts."""
import ctypes
import hashlib
import types

import numpy as np
import pytest
import torch

from simpb_amd import _lib, build, configs, plugin, synth
from tests import camera_count_cases as K
from tests import camera_dropout_ref as C
from tests import sampler_ref as S
from tests import test_samplers_float64 as T


# ---------------------------------------------------------------------------------------------------------- the entry point
def test_rig_entry_point_validates_before_any_hip_call():
    """As tests/test_capi.py::test_bad_arguments_return_einval: no device in the process."""
    build.build_extension()
    h = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)
    P = lambda n, v: [v] * n   # noqa: E731
    rig = h.simpb_dfa_fused_forward_rig
    # out, feat, is_f16, 11 pointers, bs, cams, num_feat, C, L, A, num_fix, num_learn, G, cam_valid, stream
    for cams in range(1, 9):
        assert rig(null, null, 0, *P(11, null), 2, cams, 1000, 256, 4, 77, 7, 6, 8, one, null) == 1      # NULL operands
        assert rig(one, null, 1, *P(11, one), 2, cams, 1000, 256, 4, 77, 7, 6, 8, null, null) == 1
        assert rig(one, one, 0, *P(8, one), null, one, one, 2, cams, 1000, 256, 4, 77, 7, 6, 8, null, null) == 1   # cam_logits
    for f16 in (0, 1):
        for cv in (null, one):
            assert rig(one, one, f16, *P(11, one), 2, 0, 1000, 256, 4, 77, 7, 6, 8, cv, null) == 1       # no camera
            assert rig(one, one, f16, *P(11, one), 2, 9, 1000, 256, 4, 77, 7, 6, 8, cv, null) == 1       # nine cameras
            assert rig(one, one, f16, *P(11, one), 2, -1, 1000, 256, 4, 77, 7, 6, 8, cv, null) == 1
            assert rig(one, one, f16, *P(11, one), 2, 5, 1000, 256, 3, 77, 7, 6, 8, cv, null) == 1       # num_scale = 3
            assert rig(one, one, f16, *P(11, one), 2, 5, 1000, 256, 4, 77, 6, 6, 8, cv, null) == 1       # num_fix = 6
            assert rig(one, one, f16, *P(11, one), 2, 8, 1000, 256, 4, 77, 7, 6, 4, cv, null) == 1       # num_groups = 4
            assert rig(one, one, f16, *P(11, one), 2, 8, 1000, 128, 4, 77, 7, 6, 8, cv, null) == 1       # num_embeds = 128
            assert rig(one, one, f16, *P(11, one), 0, 8, 1000, 256, 4, 77, 7, 6, 8, cv, null) == 1       # no stream
    # the two older entries keep their contract: the shipped rig only
    assert h.simpb_dfa_fused_forward_cams(one, one, 0, *P(11, one), 2, 5, 1000, 256, 4, 77, 7, 6, 8, one, null) == 1
    assert h.simpb_dfa_fused_forward(one, one, 0, *P(11, one), 2, 8, 1000, 256, 4, 77, 7, 6, 8, null) == 1
    assert h.simpb_abi_version() == 7


# ------------------------------------------------------------------------------------------- config, weights and refusals
def _head(n, **edit):
    cfg = configs.simpb_plus(anchor=synth.anchors(48), num_cams=n)["model"]["head"]
    cfg["instance_bank"].update(num_anchor=48, num_temp_instances=32)
    cfg["num_anchor"] = 48
    for path, value in edit.items():
        node = cfg
        *parents, leaf = path.split("__")
        for k in parents:
            node = node[k]
        node[leaf] = value
    return plugin.build_head(cfg).eval()


def test_config_builds_at_one_to_eight_cameras_with_the_six_camera_weights():
    six = _head(6)
    state = six.state_dict()
    want = {k: tuple(v.shape) for k, v in state.items()}
    assert configs.simpb_plus() == configs.simpb_plus(num_cams=6)          # the shipped file, key for key
    for n in range(1, 9):
        cfg = configs.simpb_plus(num_cams=n)["model"]["head"]
        assert cfg["deformable_model"]["num_cams"] == n and len(cfg["dynamic_allocation"]["limit_corners_num"]) == n
        head = _head(n)
        assert head.num_cams == n
        layers = [l for op, l in zip(head.operation_order, head.layers) if op in ("deformable", "qg_cross_attn")]
        assert len(layers) == 6 and all(l.num_cams == n for l in layers)
        assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == want, n
        head.load_state_dict(state, strict=True)


def test_rigs_that_cannot_be_served_are_refused_with_the_setting_named():
    for n in (0, 9):
        with pytest.raises(ValueError, match="num_cams"):
            _head(n)
    with pytest.raises(ValueError, match="deformable_model.num_cams"):
        _head(5, deformable_model__num_cams=6)
    with pytest.raises(ValueError, match="qg_cross_attn.num_cams"):
        _head(5, qg_cross_attn__num_cams=4)
    with pytest.raises(ValueError, match="qg_cross_attn.num_cams"):     # the class default of six against a seven-camera head
        cfg = configs.simpb_plus(anchor=synth.anchors(48), num_cams=7)["model"]["head"]
        del cfg["qg_cross_attn"]["num_cams"]
        plugin.build_head(cfg)


def test_thirteen_streams_of_eight_cameras_are_refused_where_the_runner_is_built():
    """batch * cameras <= 96 camera groups (csrc/alloc.hip): refused on the host, before anything is allocated."""
    from simpb_amd.plugin.allocation import check_stream_groups
    from simpb_amd.runner import FrameRunner
    check_stream_groups(12, 8)
    check_stream_groups(16, 6)
    with pytest.raises(ValueError, match="at most 12 streams at 8 cameras"):
        check_stream_groups(13, 8)
    model = types.SimpleNamespace(head=types.SimpleNamespace(num_cams=8))
    with pytest.raises(ValueError, match="at most 12 streams at 8 cameras"):
        FrameRunner(model, 13, (64, 176), device=torch.device("cpu"), independent_streams=True)


# --------------------------------------------------------------------------------------------------------------- synth
def test_synth_at_six_cameras_is_the_committed_ring_bit_for_bit():
    assert synth.ring(6) == (synth.CAM_YAW_DEG, synth.CAM_FOCAL)
    assert np.array_equal(synth.camera_rig((352, 128), num_cams=6), synth.camera_rig((352, 128)))
    a, b = synth.frame_metas(2, 1, (352, 128), num_cams=6), synth.frame_metas(2, 1, (352, 128))
    assert torch.equal(a["projection_mat"], b["projection_mat"]) and torch.equal(a["image_wh"], b["image_wh"])
    assert torch.equal(synth.images(1, 0, (88, 32), num_cams=6), synth.images(1, 0, (88, 32)))
    # the bytes of the ring as it was before camera_rig took a camera count (sha256 of the f32 arrays)
    assert hashlib.sha256(synth.camera_rig((704, 256), num_cams=6).tobytes()).hexdigest() == (
        "669e73a00025a8af9bb0254ba9768ec09e14d068bade85b87090795a9716b60d")
    assert hashlib.sha256(synth.frame_metas(2, 1, (176, 64), num_cams=6)["projection_mat"].numpy().tobytes()).hexdigest() == (
        "ed9c2a97129c3d6b38c9acfd763c914d498ba831e6210660e203ee1b63cfedfe")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8])
def test_synth_ring_at_n_cameras(n):
    """yaw_i = -360 * i / N, horizontal field of view min(120, 1.25 * 360 / N) degrees: a point on a camera's axis lands on
    the image centre, a point on the edge of the field of view on the image border."""
    wh = (176, 64)
    yaw, focal = synth.ring(n)
    fov = min(120.0, 450.0 / n)
    assert yaw == tuple(-360.0 * i / n for i in range(n)) and len(set(focal)) == 1
    rig = synth.camera_rig(wh, num_cams=n).astype(np.float64)
    assert rig.shape == (n, 4, 4)
    metas = synth.frame_metas(3, 0, wh, num_cams=n)
    assert tuple(metas["projection_mat"].shape) == (3, n, 4, 4) and tuple(metas["image_wh"].shape) == (3, n, 2)
    assert tuple(synth.images(2, 0, (88, 32), num_cams=n).shape) == (2, n, 3, 32, 88)
    for i in range(n):
        for off, want_u in ((0.0, wh[0] / 2), (-fov / 2, wh[0]), (fov / 2, 0.0)):     # ego y is left: a negative yaw looks right
            psi = np.radians(yaw[i] + off)
            centre = np.array([0.5 * np.cos(np.radians(yaw[i])), 0.5 * np.sin(np.radians(yaw[i])), 1.5])
            p = rig[i] @ np.append(centre + 40.0 * np.array([np.cos(psi), np.sin(psi), 0.0]), 1.0)
            assert abs(p[0] / p[2] - want_u) <= 1e-3 and abs(p[1] / p[2] - wh[1] / 2) <= 1e-3 and p[2] > 0, (i, off)


# ---------------------------------------------------------------------------- the reference alone on the GPU tests' inputs
@pytest.mark.parametrize("n", K.SEED_CAMS)
def test_oracle_on_the_ring_has_full_groups_and_no_cut_or_border_near_flipping(n, monkeypatch):
    """OracleHead at bs = 1 per stream (camera_dropout_ref.bind_cameras for the one default of six), small golden spec, three
    frames, the seeds of tests/camera_count_cases.py:
    * every camera group of every 2D layer is non-empty;
    * where neighbouring fields of view meet or overlap (N * fov >= 360 degrees: N >= 3 on this ring) the 2D set is larger
      than the anchors in view, i.e. anchors are seen by two cameras (at N = 3 the 120-degree fields only meet: boxes that
      straddle a shared border, 52 slots for 48 anchors). At N = 2 the two fields look forwards and backwards with 60 degrees
      unseen on either side, so every anchor in view has exactly one slot (39 slots for 39 anchors): "larger for N >= 2"
      cannot hold at N = 2 on this ring, and what is asserted there is the equality;
    * no ranking cut (update, cache, decode) and no projected anchor centre is within 1e-4 of flipping."""
    from oracle import simpb_ref as R
    spec = K.head_spec()
    head = K.build_head(spec, n)
    params = {k: v.detach() for k, v in head.state_dict().items()}
    C.bind_cameras(monkeypatch, range(n))
    overlap = n * min(120.0, 450.0 / n) >= 360.0
    for b in range(K.HEAD_BS):
        oracle = R.OracleHead(params, head.operation_order, spec["num_anchor"], spec["num_temp"], spec["num_output"])
        for f in range(K.HEAD_FRAMES):
            maps, metas = K.frame_inputs(spec, n, f)
            fm, one = R.feature_maps_format(maps), K.one_stream(metas, b)
            with torch.no_grad():
                want = oracle.forward([fm[0][b:b + 1], fm[1], fm[2]], one)
            m = K.margins(want, oracle, one, spec, f > 0)
            sizes = [[hi - lo for lo, hi in g] for g in want["ref_query_groups_list"]]
            n2 = [t.shape[1] for t in want["ref_trans_matrix_list"]]
            seen = [int((t[0].sum(0) > 0).sum()) for t in want["ref_trans_matrix_list"]]
            print(f"FIG N{n} stream {b} frame {f} margins={ {k: f'{v:.1e}' for k, v in m.items()} } smallest_group={min(map(min, sizes))} "
                  f"slots={n2} anchors_in_view={seen}")
            assert all(len(g) == n for g in sizes) and min(map(min, sizes)) >= 1, (b, f, sizes)
            if overlap:
                assert all(a > s for a, s in zip(n2, seen)), (b, f, n2, seen)
            else:
                assert n2 == seen, (b, f, n2, seen)
            assert min(m.values()) >= K.NEAR, (b, f, m)


@pytest.mark.parametrize("n", K.OPS_CAMS)
def test_operator_cases_leave_the_gate_decided(n):
    """The float64 statement alone on the operator cases of tests/test_gpu_camera_count_ops.py, every mask: at most 2 % of the
    anchors carry a sample whose gate the fp32 error could flip (they are left out of the gate comparison), enough samples
    are valid, and in the scene samples lie behind a camera (depth <= 1e-5: the clamp engages)."""
    for family, kind in K.OPS_CASES:
        c = K.ops_case(n, family, kind)
        for mask_kind in K.MASKS:
            mask = K.mask_of(mask_kind, n)
            pts = K.masked_points(c, mask)
            und, left = K.anchors_left_out(pts, mask)
            on = np.ones((c["bs"], n), bool) if mask is None else mask != 0
            valid = int((T.gate(pts["loc"]) & on[:, None, None, :]).sum())
            clamped = int(((pts["depth"] <= 1e-5) & on[:, None, None, :]).sum())
            print(f"FIG N{n} {family} {kind} {mask_kind} valid={valid} clamped={clamped} undecided={int(und.sum())} "
                  f"anchors_left_out={left} of {c['bs'] * c['A']}")
            assert left <= 0.02 * c["bs"] * c["A"] and valid >= 200
            if family == "scene":
                assert clamped >= 30
        assert mask is not None and (mask.sum(1) == 1).all()           # "one_left": one camera per stream ...
        assert n < 3 or len({int(r.argmax()) for r in mask}) == 3      # ... another one in every stream


def test_fp32_oracle_stays_under_half_of_the_bounds_at_n_cameras():
    """The recipe of tests/test_samplers_float64.py::test_fp32_oracle_stays_under_half_of_the_bounds on the N-camera cases: the
    fp32 oracle's aggregation on the float64 operands rounded to fp32, its figure against (b) and the kappa it needs for (e).
    That module's KAPPA = 1.7 covers them (measured: kappa 0.00 at every N -- half of grad_sum alone covers the oracle's
    error, as on the six-camera 3D cases)."""
    worst_b, worst_k = 0.0, 0.0
    for n in K.OPS_CAMS:
        for family, kind in K.OPS_CASES:
            c = K.ops_case(n, family, kind)
            loc = c["points"]["loc"].astype(np.float32)
            w = S.dfa_weights(c["fl"], c["cl"], K.LVL, K.NPTS, K.GRP).astype(np.float32)
            got = T.oracle_daf(c["col"], c["ss"], c["st"], loc, w)
            want, ab, gr = S.daf(c["col"], c["ss"], c["st"], loc, w)
            b, k = S.bound_b(got, want), S.kappa_needed(got, want, ab, gr)
            print(f"FIG oracle N{n} {family} {kind} b={b:.3f} e={T.figures(got, want, ab, gr)[1]:.3f} kappa={k:.2f}")
            worst_b, worst_k = max(worst_b, b), max(worst_k, k)
    print(f"FIG oracle worst b={worst_b:.3f} kappa={worst_k:.2f} KAPPA={T.KAPPA}")
    assert worst_b <= 0.5
    assert 2 * worst_k <= T.KAPPA, (worst_k, T.KAPPA)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_token_buffer_of_n_cameras_is_row_major(n):
    """ops.feature_maps_format at n cameras equals the oracle's formatter and is contiguous: at ONE camera the reference's
    permute + flatten is a view of the permuted tensor, which the kernels (and ops.dfa_fused's check) do not take."""
    from oracle import simpb_ref as R
    from simpb_amd.plugin import ops
    maps = synth.feature_maps_nchw(2, 0, (88, 32), channels=16, num_cams=n)
    got, want = ops.feature_maps_format(maps), R.feature_maps_format(maps)
    assert got[0].is_contiguous() and torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]) and tuple(got[1].shape) == (n, 4, 2)
