"""GPU: the 2D records of a rig whose cameras differ in crop and resize (csrc/decode.hip: simpb_decode2d_record_cams,
simpb_decode2d_record_ragged_cams). They are the scalar entry points with a per-camera table in place of the four scalars,
so the scalar entry points are the witness: every row equals, bit for bit, the row the scalar entry point writes when it is
called with the four numbers of that row's camera. No tolerance and no host formula."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C, A, K = 3, 37, 20
N2_SIZES = (1, 255, 257)
# (crop, resize) of three cameras that differ in every number
RULES = (((0, 140, 704, 396), 0.44), ((70, 140, 774, 396), 0.55), ((5, 3, 645, 243), 1.0 / 3.0))


def api():
    from simpb_amd import _lib as L
    from simpb_amd.plugin.ops import _ptr, _stream
    return L, L.lib(), _ptr, _stream


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def table(rules):
    """f32 [cams, 4] as preprocess.RigPlan.box2d_table makes it."""
    return np.asarray([(c[2] - c[0], c[3] - c[1], c[1], np.float32(1.0) / np.float32(r)) for c, r in rules], np.float32)


def scalars(rule):
    crop, resize = rule
    return float(crop[2] - crop[0]), float(crop[3] - crop[1]), float(crop[1]), float(resize)


def static_case(n2):
    rng = np.random.default_rng([11, n2])
    bs = 2
    d = dict(cls2d=rng.standard_normal((bs, n2, C)).astype(np.float32) * 3, box2d=rng.uniform(-0.2, 1.2, (bs, n2, 4)).astype(np.float32),
             q2a=rng.integers(-1, A + 1, (bs, n2)).astype(np.int32), cam=rng.integers(-1, 3, n2).astype(np.int32),
             rank=rng.integers(-1, K, (bs, A)).astype(np.int32))
    return {k: dev(v) for k, v in d.items()}, d["cam"]


def run_static(d, n2, rule=None, rules=None):
    L, lib, P, S = api()
    rec = torch.full((2, n2, 8), -7.0, device="cuda")
    ins = [P(d[k]) for k in ("cls2d", "box2d", "q2a", "cam", "rank")]
    if rules is None:
        L.check(lib.simpb_decode2d_record(P(rec), *ins, 2, n2, C, A, *scalars(rule), S()), "simpb_decode2d_record")
    else:
        t = dev(table(rules))
        L.check(lib.simpb_decode2d_record_cams(P(rec), *ins, 2, n2, C, A, P(t), len(rules), S()), "simpb_decode2d_record_cams")
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("n2", N2_SIZES)
def test_static_record_follows_each_slots_camera(n2):
    d, cam = static_case(n2)
    for rule in RULES:      # equal rows: the scalar entry point's bits
        assert np.array_equal(run_static(d, n2, rules=[rule] * 3), run_static(d, n2, rule=rule))
    got = run_static(d, n2, rules=RULES)
    per_rule = [run_static(d, n2, rule=rule) for rule in RULES]
    pick = np.clip(cam, 0, 2)       # (an empty slot, camera -1, takes row 0: its box is never looked at)
    for slot in range(n2):
        assert np.array_equal(got[:, slot], per_rule[pick[slot]][:, slot]), (slot, cam[slot])
    if n2 > 1:
        assert any(not np.array_equal(got, p) for p in per_rule)


def ragged_case(rows):
    """Three streams of rows + 1 (one slot more than the record has rows), 0 and rows - 1 slots, three cameras each."""
    rng = np.random.default_rng([12, rows])
    bs, cams = 3, 3
    counts = (rows + 1, 0, rows - 1)
    group_start, stream_of, cam_of = [0], [], []
    for b, n in enumerate(counts):
        for cam, m in enumerate((n // 3, n // 3, n - 2 * (n // 3))):
            group_start.append(group_start[-1] + m)
            stream_of += [b] * m
            cam_of += [b * cams + cam] * m
    s = max(group_start[-1], 1)
    q2a = rng.integers(0, A, s).astype(np.int32) + (np.asarray(stream_of + [0] * (s - len(stream_of)), np.int32)) * A
    q2a[3::5], q2a[4::7] = -1, bs * A
    d = dict(cls2d=rng.standard_normal((s, C)).astype(np.float32) * 3, box2d=rng.uniform(-0.2, 1.2, (s, 4)).astype(np.float32), q2a=q2a,
             cam=np.asarray(cam_of + [0] * (s - len(cam_of)), np.int32), group_start=np.asarray(group_start, np.int32),
             rank=rng.integers(-1, K, (bs, A)).astype(np.int32))
    return {k: dev(v) for k, v in d.items()}


def run_ragged(d, rows, rule=None, rules=None):
    L, lib, P, S = api()
    rec = torch.full((3, rows, 8), -7.0, device="cuda")
    ins = [P(d[k]) for k in ("cls2d", "box2d", "q2a", "cam", "group_start", "rank")]
    if rules is None:
        L.check(lib.simpb_decode2d_record_ragged(P(rec), *ins, 3, rows, 3, C, A, *scalars(rule), S()), "simpb_decode2d_record_ragged")
    else:
        t = dev(table(rules))
        L.check(lib.simpb_decode2d_record_ragged_cams(P(rec), *ins, 3, rows, 3, C, A, P(t), S()), "simpb_decode2d_record_ragged_cams")
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("rows", N2_SIZES)
def test_ragged_record_follows_each_slots_camera(rows):
    d = ragged_case(rows)
    for rule in RULES:
        assert np.array_equal(run_ragged(d, rows, rules=[rule] * 3), run_ragged(d, rows, rule=rule))
    got = run_ragged(d, rows, rules=RULES)
    per_rule = [run_ragged(d, rows, rule=rule) for rule in RULES]
    cam = per_rule[0].view(np.float32)[..., 7]          # the record's own camera column (-1: a pad row, equal in every run)
    for b in range(3):
        for r in range(rows):
            want = per_rule[int(max(cam[b, r], 0))]
            assert np.array_equal(got[b, r], want[b, r]), (b, r, cam[b, r])
    if rows > 1:
        assert any(not np.array_equal(got, p) for p in per_rule)


def test_refusals():
    L, lib, P, S = api()
    d, _ = static_case(5)
    rec = torch.full((2, 5, 8), -7.0, device="cuda")
    ins = [P(d[k]) for k in ("cls2d", "box2d", "q2a", "cam", "rank")]
    t = dev(table(RULES + RULES[:1]))
    assert lib.simpb_decode2d_record_cams(P(rec), *ins, 2, 5, C, A, None, 3, S()) == 1
    assert lib.simpb_decode2d_record_cams(P(rec), *ins, 2, 5, C, A, P(t), 0, S()) == 1
    assert lib.simpb_decode2d_record_cams(P(rec), *ins, 2, 5, C, A, P(t.view(-1)[1:]), 3, S()) == 1      # a table off the 16-byte grid
    g = dev(np.zeros(7, np.int32))
    assert lib.simpb_decode2d_record_ragged_cams(P(rec), *ins[:4], P(g), ins[4], 2, 5, 3, C, A, None, S()) == 1
    torch.cuda.synchronize()
    assert bool((rec == -7.0).all())
