"""CPU: the host model of tests/alloc_ref.py against the reference's own vectors (tests/golden/ops.npz alloc.*, the first
allocation of head_r50.npz) and against oracle/simpb_ref.py::allocation run in float32 on decided inputs with corner-only slots
and bs > 1; every generator tests/test_allocation_exact.py uses, with the guards they assert themselves (decidedness, the
redraw cap, the counts a pattern names) and a check that the edges they are meant to contain are really in what they generate
and really computed without rounding; and the three forms of `tables` against each other."""
import numpy as np
import torch

from simpb_amd import synth
from tests import alloc_ref as R
from tests import test_allocation_exact as X
from tests.helpers import load_golden, spec_of

# the oracle evaluates the same statements in float32: under twenty roundings of one unit each (alloc_ref's module docstring)
ORACLE_UNITS = 20.0


def onehot(q2a, A, gate=None):
    out = np.zeros(q2a.shape + (A,), np.float32)
    for b, s in np.argwhere(q2a >= 0):
        out[b, s, q2a[b, s]] = 1.0 if gate is None else float(gate[b, s])
    return out


# ------------------------------------------------------------------------------------------- the model and the reference vectors
def test_model_reproduces_the_reference_case_of_ops_npz():
    g = load_golden("ops.npz")
    proj = synth.frame_metas(1, 0)["projection_mat"].numpy()
    p = R.project(g["alloc.anchor"], proj, X.IMG_WH)
    t = R.tables(p["flag"], p["sel"], p["depth"], X.IMG_WH, "exact")
    assert np.array_equal(t["q2a"], g["alloc.q2a"]) and np.array_equal(t["is_center"], g["alloc.is_center"])
    assert np.array_equal((p["flag"] != 0).transpose(0, 2, 1), g["alloc.trans_mask"])
    assert np.array_equal(t["count"], g["alloc.trans_shape"])
    assert np.array_equal(np.stack([t["group_start"][:-1], t["group_start"][1:]], 1), g["alloc.query_groups"])
    assert np.abs(t["ref_pts2d"] - g["alloc.ref_pts2d"]).max() <= 1e-6       # (tests/test_gpu_golden_ops.py's tolerances)
    assert np.abs(t["ref_depth2d"][..., None] - g["alloc.ref_depth2d"]).max() <= 1e-5


def test_model_reproduces_the_first_allocation_of_the_r50_frame():
    g = load_golden("head_r50.npz")
    spec = spec_of(g)
    G = lambda k: g[f"f0.trace.L00.allocation.{k}#0"]  # noqa: E731
    anchor = synth.anchors(spec["num_anchor"])[None]             # the learned table of a cold bank (tests/helpers.py)
    proj = synth.frame_metas(1, 0, spec["image_wh"])["projection_mat"].numpy()
    p = R.project(anchor, proj, spec["image_wh"])
    t = R.tables(p["flag"], p["sel"], p["depth"], spec["image_wh"], "exact")
    assert np.array_equal((p["flag"] != 0).transpose(0, 2, 1).astype(np.uint8), G("trans_mask"))
    assert np.array_equal(t["q2a"], G("q2a")) and np.array_equal(t["is_center"], G("is_center"))
    assert np.array_equal(t["count"], G("trans_shape"))
    assert np.array_equal(np.stack([t["group_start"][:-1], t["group_start"][1:]], 1), G("query_groups"))
    assert np.abs(t["ref_pts2d"] - G("ref_pts2d")).max() <= 1e-5
    assert np.abs(t["ref_depth2d"][..., None] - G("ref_depth2d")).max() <= 1e-5 * np.abs(G("ref_depth2d")).max()


# ----------------------------------------------------------------------------------------------------- the model and the oracle
def oracle(anchor, proj):
    from oracle import simpb_ref
    bs, cams = proj.shape[:2]
    metas = dict(projection_mat=torch.from_numpy(proj), image_wh=torch.tensor([float(X.IMG_WH[0]), float(X.IMG_WH[1])]).view(1, 1, 2).repeat(bs, cams, 1))
    with torch.no_grad():
        return simpb_ref.allocation(torch.from_numpy(anchor), metas)


def agree_with_oracle(g, units):
    p = g["p"]
    pts, depth, mask, shape, trans, cmat, groups = oracle(g["anchor"], g["proj"])
    t = R.tables(p["flag"], p["sel"], p["depth"], X.IMG_WH, "exact", size_sel=p["size_sel"], size_depth=p["size_depth"])
    A = g["anchor"].shape[1]
    assert np.array_equal(mask.numpy(), (p["flag"] != 0).transpose(0, 2, 1))
    assert np.array_equal(shape.numpy(), t["count"])
    assert [list(x) for x in groups] == np.stack([t["group_start"][:-1], t["group_start"][1:]], 1).tolist()
    assert np.array_equal(trans.numpy(), onehot(t["q2a"], A)) and np.array_equal(cmat.numpy(), onehot(t["q2a"], A, t["is_center"]))
    assert X.units(pts.numpy(), t["ref_pts2d"], t["size_pts"]) <= units
    assert X.units(depth.numpy()[..., 0], t["ref_depth2d"], t["size_depth"]) <= units
    return t


def test_model_agrees_with_the_float32_oracle_on_decided_rigs():
    for bs, A in ((1, 1), (2, 65), (3, 257)):
        g = X.random_rig(bs, A, 0)
        t = agree_with_oracle(g, ORACLE_UNITS)
        if A > 1:
            live = t["q2a"] >= 0
            assert (t["is_center"][live] == 0).sum() >= 10 and (t["is_center"][live] == 1).sum() >= 10     # corner-only slots
            assert bs == 1 or (~live).any()                                                             # pads inside groups
    agree_with_oracle(X.random_rig(2, 65, 1, 8), ORACLE_UNITS)


def test_model_agrees_with_the_float32_oracle_on_the_lattice():
    """On the border cases nothing rounds (test_lattice_points_are_exact_in_float32), so the float32 oracle must make the
    model's decisions there, with the model's numbers."""
    for cams in (6, 8):
        agree_with_oracle(X.lattice_rig(cams), ORACLE_UNITS)


# ------------------------------------------------------------------------------------------------------------------ generators
def test_random_rigs_are_decided_and_hold_what_they_are_for():
    for args in ((1, 1, 0), (2, 65, 0), (3, 257, 0), (16, 64, 0), (16, 600, 0), (2, 65, 1, 8), (2, 65, 3), (2, 65, 3, 8)):
        g = X.random_rig(*args)                         # asserts decidedness and the redraw cap itself
        p = g["p"]
        assert R.undecided(p) == [] and g["redrawn"] < 0.01 * p["flag"][:, 0].size
        if args[1] == 1:
            continue
        count, _ = R.compact(p["flag"])
        assert len({tuple(c) for c in count.tolist()}) == args[0]                        # per-camera counts differ between streams
        assert (p["flag"] == 1).any() and (p["flag"] == 2).any() and (p["flag"] == 0).any()
        assert ((p["d"][..., :8] <= 0).any(-1) & (p["flag"] == 1)).any()                 # flagged by a corner, others behind the camera
        assert (g["anchor"][..., 3] > np.log(35.0)).any() and (g["anchor"][..., 5] > np.log(10.0)).any()
        assert (g["anchor"][..., 3] < np.log(35.0)).any()
        assert (np.hypot(g["anchor"][..., 0], g["anchor"][..., 1]) < 2.0).mean() > 0.1


def case(g, name, turn=0):
    """(stream 0, camera 0) of a lattice case: its anchor index and the model's points."""
    a = turn * len(X.LATTICE_CASES) + g["names"].index(name)
    return a, {k: g["p"][k][0, 0, a] for k in ("x", "y", "d", "flag", "sel", "depth")}


def test_lattice_points_are_exact_in_float32():
    """The waiver of the margin: every quantity within 64 roundings of a threshold is computed without any rounding (or is one
    correctly rounded division of two such numbers, far enough from the threshold for that one rounding), and the statements
    evaluated in float32 make every decision of the float64 model."""
    w, h = X.IMG_WH
    for cams in (6, 8):
        g = X.lattice_rig(cams)
        p, waive = g["p"], g["waive"]
        R.assert_decided(p, waive)
        assert R.undecided(p) != []                                  # without the waiver the lattice is not decided: it sits on the borders
        p32 = R.project(g["anchor"], g["proj"], X.IMG_WH, dtype=np.float32)
        assert np.array_equal(p32["flag"], p["flag"])
        near = p["margin_q"] < R.DECIDED
        assert near.any() and (waive[..., :3] | (waive[..., [3, 4, 2]] & waive[..., 2:3]))[near].all()
    g = X.lattice_rig()
    for turn in (0, 1):
        for name, axis, value in (("x_eq_0", "x", 0.0), ("x_eq_w", "x", w), ("y_eq_0", "y", 0.0), ("y_eq_h", "y", h)):
            a, c = case(g, name, turn)
            assert c[axis][8] == value and g["waive"][0, 0, a, 8, :3].all() and c["flag"] == 1
            _, c = case(g, name + "_inside", turn)
            assert abs(c[axis][8] - value) == 1.0 and c["flag"] == 2 and np.array_equal(c["sel"], [c["x"][8], c["y"][8]])
            # the same border met by a corner with d > 0 that is otherwise inside, every other point outside
            a, c = case(g, "corner_" + name, turn)
            on = np.flatnonzero(c[axis][:8] == value)
            other = "y" if axis == "x" else "x"
            assert len(on) >= 1 and g["waive"][0, 0, a, on, :3].all() and (c["d"][on] > 0).all() and c["flag"] == 0
            assert ((0 < c[other][on]) & (c[other][on] < (h if axis == "x" else w))).all()
            _, c = case(g, "corner_" + name + "_inside", turn)
            assert (np.abs(c[axis][:8] - value) == 1.0).sum() == len(on) and c["flag"] == 1


def test_lattice_depth_cases_are_what_they_are_named():
    w, h = X.IMG_WH
    g = X.lattice_rig()
    inside = lambda c: (0 < c["x"][:8]) & (c["x"][:8] < w) & (0 < c["y"][:8]) & (c["y"][:8] < h)  # noqa: E731
    for turn in (0, 1):
        _, c = case(g, "corner_d_eq_0", turn)
        assert (inside(c) & (c["d"][:8] == 0)).sum() == 1 and not (inside(c) & (c["d"][:8] > 0)).any() and c["flag"] == 0
        _, c = case(g, "corner_d_below_0", turn)
        assert (inside(c) & (c["d"][:8] < 0)).sum() == 1 and not (inside(c) & (c["d"][:8] > 0)).any() and c["flag"] == 0
        _, c = case(g, "corner_d_clear", turn)
        assert (inside(c) & (c["d"][:8] > R.CLAMP)).sum() == 1 and c["flag"] == 1
        _, c = case(g, "corner_d_below_clamp", turn)
        assert (inside(c) & (c["d"][:8] > 0) & (c["d"][:8] < R.CLAMP)).sum() == 1 and c["flag"] == 1
        _, c = case(g, "centre_behind_inside", turn)
        assert c["d"][8] == -X.E20 and c["flag"] == 2 and c["depth"] == -X.E20 and np.array_equal(c["sel"], [c["x"][8], c["y"][8]])
        assert 0 < c["x"][8] < w and 0 < c["y"][8] < h and c["x"][8] == c["sel"][0]
        _, c = case(g, "centre_below_clamp", turn)
        assert 0 < c["d"][8] < R.CLAMP and c["flag"] == 2
        _, c = case(g, "straddle", turn)
        assert not ((c["d"][:8] > 0) & inside(c)).any() and c["flag"] == 0
        assert c["x"][:8].min() < 0 and c["x"][:8].max() > w and c["y"][:8].min() < 0 and c["y"][:8].max() > h
        assert np.array_equal(c["sel"], [w / 2, h / 2])                # the clamped box centre lies inside: still no query
        _, c = case(g, "both_sides_clamped", turn)
        assert c["flag"] == 1 and c["x"][:8].min() < 0 and c["x"][:8].max() > w and c["sel"][0] == w / 2
        assert 0 < c["y"][:8].max() < h and c["sel"][1] == c["y"][:8].max() / 2
    for i, (name, _, _, want) in enumerate(X.LATTICE_CASES):            # stream 1: reversed anchors, camera 0's matrix in place 1
        assert g["p"]["flag"][0, 0, i] == want == g["p"]["flag"][1, 1, 2 * len(X.LATTICE_CASES) - 1 - i], name


def test_count_patterns_produce_the_patterns_they_name():
    for name, counts, _ in X.COUNT_PATTERNS:
        g = X.count_pattern(name)                        # asserts the model's counts and decidedness itself
        counts = np.asarray(counts)
        p = g["p"]
        st = R.tables(p["flag"], p["sel"], p["depth"], X.IMG_WH, "static", g["capacity"])
        rg = R.tables(p["flag"], p["sel"], p["depth"], X.IMG_WH, "ragged", g["per_stream"])
        total = int(counts.max(0).sum())
        if name == "empty_first_and_last":
            assert counts[0, 0] == 0 and counts[0, -1] == 0 and st["group_start"][1] == 0 and st["group_start"][-1] == st["group_start"][-2]
        if name == "one_camera_holds_all":
            assert (p["flag"][0, 2] == 2).all() and counts.sum() == counts[0, 2] == g["anchor"].shape[1]
        if name == "a_stream_without_any":
            assert not p["flag"][1].any() and (rg["group_start"][6:13] == rg["group_start"][6]).all() and (st["q2a"][1] == -1).all()
        if name == "total_eq_capacity":
            assert g["capacity"] == total and st["overflow"] == 0 and (st["query_cam"] >= 0).all()
            assert g["per_stream"] == counts.sum(1).max() and rg["overflow"] == 0
        if name == "total_eq_capacity_plus_1":
            assert g["capacity"] == total - 1 and st["overflow"] == 1 and (st["query_cam"] >= 0).all()
            assert rg["overflow"] == 1 and (rg["a2q"] >= 0).sum() == counts.sum() - 1
        if name == "first_camera_above_capacity":
            assert g["capacity"] < counts[:, 0].max() and st["overflow"] == 1 and (st["group_start"][1:] == g["capacity"]).all()
            assert (st["a2q"][:, :, 1:] == -1).all() and rg["overflow"] == 1
        if name == "maxima_in_other_streams":
            assert counts.argmax(0).tolist() == [0, 1, 2, 0, 1, 2] and (st["q2a"][:, :total] == -1).any()
        assert X.capacities(counts)[:2] == [total, total - 1]


def test_compaction_and_aggregate_cases_hold_what_they_are_for():
    for A in X.COMPACT_A:
        flag = X.compact_case(A)
        count, order = R.compact(flag)
        assert flag.shape == (1, 6, A) and count[0].tolist() == [0, A, 1, 1, (A + 1) // 2, min(A, 64)]
        assert order[0][3].tolist() == [A - 1] and set(np.unique(flag)) <= {0, 1, 2} and (A < 4 or {1, 2} <= set(np.unique(flag[0, 1])))
    for cams in (X.CAMS, 8):
        for C in X.AGG_CHANNELS:
            for kind in ("alpha", "tiny", "hidden", "hidden_low"):
                X.aggregate_case(cams, C, kind)            # asserts 0 / 1 / >= 3 slots, pads and the clamp itself


# ---------------------------------------------------------------------------------------------------------------- tables forms
def test_static_form_with_room_is_the_exact_form_plus_pads():
    for g in (X.random_rig(3, 257, 0), X.count_pattern("maxima_in_other_streams"), X.lattice_rig()):
        p = g["p"]
        ex = R.tables(p["flag"], p["sel"], p["depth"], X.IMG_WH, "exact")
        n = ex["n2"]
        for room in (0, 9):
            st = R.tables(p["flag"], p["sel"], p["depth"], X.IMG_WH, "static", n + room)
            assert st["overflow"] == 0 and np.array_equal(st["group_start"], ex["group_start"]) and np.array_equal(st["a2q"], ex["a2q"])
            for k in ("q2a", "is_center", "ref_pts2d", "ref_depth2d"):
                assert np.array_equal(st[k][:, :n], ex[k]) and (st[k][:, n:] == (-1 if k == "q2a" else 0)).all(), k
            assert np.array_equal(st["query_cam"][:n], ex["query_cam"]) and (st["query_cam"][n:] == -1).all()


def test_ragged_form_is_every_stream_as_a_batch_of_one():
    for g, per_stream in ((X.random_rig(3, 257, 0), 400), (X.random_rig(3, 257, 0), 150), (X.count_pattern("a_stream_without_any"), 20)):
        p = g["p"]
        bs, cams, A = p["flag"].shape
        rg = R.tables(p["flag"], p["sel"], p["depth"], X.IMG_WH, "ragged", per_stream)
        over = 0
        for b in range(bs):
            one = R.tables(p["flag"][b:b + 1], p["sel"][b:b + 1], p["depth"][b:b + 1], X.IMG_WH, "static", per_stream)
            over |= one["overflow"]
            lo, hi = rg["group_start"][b * cams], rg["group_start"][(b + 1) * cams]
            n = one["group_start"][-1]
            assert hi - lo == n and np.array_equal(rg["group_start"][b * cams:(b + 1) * cams + 1] - lo, one["group_start"])
            assert np.array_equal(rg["q2a"][0, lo:hi], one["q2a"][0, :n] + b * A) and np.array_equal(rg["is_center"][0, lo:hi], one["is_center"][0, :n])
            assert np.array_equal(rg["query_cam"][lo:hi], one["query_cam"][:n] + b * cams)
            assert np.array_equal(rg["ref_pts2d"][0, lo:hi], one["ref_pts2d"][0, :n]) and np.array_equal(rg["ref_depth2d"][0, lo:hi], one["ref_depth2d"][0, :n])
            assert np.array_equal(np.where(rg["a2q"][b] >= 0, rg["a2q"][b] - lo, -1), one["a2q"][0])
        assert rg["overflow"] == over and (rg["q2a"][0, rg["group_start"][-1]:] == -1).all() and (rg["query_cam"][rg["group_start"][-1]:] == -1).all()


def test_aggregate_model_is_the_statement_in_torch_float64():
    """aggregation.py:32-35 word for word on float64 tensors, with the one-hot matrix of the model's q2a."""
    for kind in ("alpha", "tiny", "hidden_low"):
        d, (out_q, out_pos, _, _, total) = X.aggregate_case(X.CAMS, 4, kind)
        T = lambda x: torch.from_numpy(np.asarray(x, np.float64))  # noqa: E731
        if d["alpha"] is not None:
            alpha = T(d["alpha"])[..., None]
        else:
            alpha = torch.sigmoid(T(d["hidden"]) @ T(d["weight"])[:, None] + float(d["bias"]))
        rw = (T(onehot(d["q2a"], 65)) * alpha).permute(0, 2, 1)
        div = torch.clamp(rw.sum(-1).unsqueeze(-1), float(np.float32(1e-5)))
        assert np.allclose(out_q, (T(d["q3d"]) + torch.matmul(rw, T(d["q2d"])) / div).numpy(), rtol=1e-12, atol=0)
        assert np.allclose(out_pos, (T(d["pos3d"]) + torch.matmul(rw, T(d["pos2d"])) / div).numpy(), rtol=1e-12, atol=0)
        assert np.allclose(total, rw.sum(-1).numpy(), rtol=1e-12, atol=0)
        src = d["q3d"]
        assert np.array_equal(R.gather(src, d["q2a"]), np.einsum("bsa,bac->bsc", onehot(d["q2a"], 65), src))
