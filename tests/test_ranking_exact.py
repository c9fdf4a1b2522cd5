"""GPU: the kernels that decide WHICH boxes leave the decoder and WHICH track id each one carries -- csrc/rowops.hip
topk_rows_kernel<512|1024|2048>, csrc/decode.hip decode3d / decode2d / decode2d_ragged, csrc/bank.hip get / update_rank /
merge / cache / cache_streams / gather -- against the plain float64 host model of tests/rank_ref.py, through the C entry
points, at the smallest shapes at which each kernel can still go wrong (both sides of every template switch, no pad / one
pad / almost only pads in the 1024-key sorts, K = A, T = A, one fresh row, A - 1 fresh rows).

The outputs are discrete (indices, labels, ranks, int64 ids), so the inputs are built such that the expected order is
decided by the mathematics and not by how the device rounds an exponential:
  * class logits are multiples of 0.25 in [-5, 5], quality logits come from QUALITY, previous confidences are lattice
    sigmoids times 0.6^j: any two scores that meet in a ranking are bit-equal (same inputs, or the commutative swap
    sigmoid(a) * sigmoid(b)) or differ by more than 1e-5 relative in float64 (rank_ref.assert_separated; every generator
    below asserts it on what the model ranked, and tests/test_rank_ref_host.py runs every generator without a GPU);
  * ties on purpose: many anchors on one lattice point, copied and rolled rows (one maximum in different columns), rows of
    one value only ("flat");
  * saturation: rows with two different logits >= 20, the smaller one in the lower column -- both sigmoids are exactly 1.0f,
    the label is the lower column (torch.max on the sigmoids), the argmax of the logits is the other one; rows of logits
    <= -1e4 whose score is exactly +0.0 and which must still outrank every pad key of the sort;
  * the id threshold 0.5 meets maximum logits of exactly 0 (score exactly 0.5: an id is issued) and of -0.25 (none).

Every output lies inside a larger sentinel-filled buffer that is checked after the launches. Scores are compared with the
model within 8 fp32 ulp (SCORE_BOUND); the exp / atan2 box columns and the pixel columns within four times the worst error
measured over this module (profiles/ranking_vs_float64.md); every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

from tests import rank_ref as R

gpu = pytest.mark.gpu

C, E = 3, 8
CROP, RESIZE = (0, 140, 704, 396), 0.44
QUALITY = np.array([-2.0, -0.75, 0.0, 0.5, 1.25, 3.0], np.float32)
DECODE_ID_BASE = ((1 << 24) + 1, (1 << 40) + 3)            # above 2^24 (float32 stops being exact) and above 2^32
BANK_ID_BASE = ((1 << 24) + 1, (1 << 33) + 7, (1 << 36) + 5)
PREV_ID = (1 << 40) + 3
MAX_DT, DEFAULT_DT, DECAY, THRESHOLD = 2.0, 0.5, 0.6, 0.5

# relative to the model value: one expf, one add, one correctly rounded divide (and a second sigmoid and a multiply)
SCORE_BOUND = 8 * R.ULP
# absolute, four times the worst error measured over every case of this module (profiles/ranking_vs_float64.md: 1.63e-6 on
# exp(w, l, h), 2.84e-7 on atan2, 1.63e-4 on pixels up to 1600); the 2e-4 / 2e-3 of
# tests/test_dense.py::test_fused_decode_records_match_the_pytorch_statement are 30 / 175 / 3 times wider
EXP_BOUND, ATAN2_BOUND = 6.6e-6, 1.2e-6
PIXEL_BOUND = 6.6e-4
# bank_get: a column is a sum of at most four products of a rounded operand: at most 8 roundings of 2^-24 each, relative to
# the sum of the magnitudes of its terms (rank_ref.bank_get "size")
WARP_BOUND = 8 * 2.0 ** -24

SAT_A, SAT_B, SAT_C = (20.0, 25.0, -3.0), (-3.0, 20.0, 25.0), (20.0, 0.5, 25.0)   # label 0 / 1 / 0, argmax of the logits 1 / 2 / 2
ZERO = (-2e4, -1e4, -1e4)                                                          # score exactly +0.0, label 0
HALF, BELOW = (0.0, -1.0, -2.5), (-0.25, -0.25, -3.0)                              # score exactly 0.5 / the next lattice point
SPECIALS = ("sat_a", "zero", "copy", "half", "sat_b", "roll", "below", "sat_c")


def note(name, value):
    print(f"FIG {name} {value:.4g}")


# ================================================================================================================ generators
def class_rows(rng, n, mode="mixed", dim=0.0):
    """f32 [n, C] lattice logits. mixed (n >= 5): up to n / 4 rows (at least 8 where there are that many) are replaced by the
    SPECIALS in turn; row 0 is the source of the copied / rolled rows. dim: that share of the rows is moved down by 4 first
    (more scores below the id threshold). flat: every row is row 0."""
    rows = (rng.integers(-20, 21, (n, C)) * 0.25).astype(np.float32)
    sel = rng.random(n) < dim
    rows[sel] = np.maximum(rows[sel] - 4.0, -5.0)
    if mode == "flat":
        rows[:] = rows[0]
    elif n >= 5:
        first = rows[0].copy()
        kinds = dict(sat_a=SAT_A, sat_b=SAT_B, sat_c=SAT_C, zero=ZERO, half=HALF, below=BELOW, copy=first, roll=np.roll(first, 1))
        for i, a in enumerate(1 + rng.permutation(n - 1)[:max(8, n // 4)]):
            rows[a] = kinds[SPECIALS[i % len(SPECIALS)]]
    return rows


def some_ranks(rng, bs, A, K):
    """A rank_of_anchor table as decode3d leaves it: K anchors per stream hold the ranks 0 .. K - 1, the others -1."""
    rank = np.full((bs, A), -1, np.int32)
    for b in range(bs):
        rank[b, rng.permutation(A)[:K]] = np.arange(K)
    return rank


def slot_anchors(rng, shape, A):
    """q2a: anchors in range, and -1, A and A + 5 (no anchor) in between."""
    q = rng.integers(0, A, shape).astype(np.int32)
    flat = q.reshape(-1)
    flat[3::5], flat[4::7], flat[6::11] = -1, A, A + 5
    return q


# ---------------------------------------------------------------------------------------------------------------------- top-k
TOPK_N = (1, 2, 511, 512, 513, 1024, 1025, 2047, 2048)   # both sides of the 512- and the 1024-key template


def topk_case(n):
    """Three rows: lattice values with ties, -inf and signed zeros (a -0.0 in front of and behind a +0.0) | all equal (odd
    n: 0.5; even n: zeros of alternating sign) | continuous values with -inf. Returns (scores, {k: model index})."""
    rng = np.random.default_rng([7, n])
    x = np.empty((3, n), np.float32)
    x[0] = rng.integers(-6, 7, n) * 0.5
    x[1] = 0.5
    x[2] = rng.standard_normal(n)
    x[2, 0] = -np.inf
    if n >= 2:
        x[0, 0], x[0, 1] = -0.0, 0.0
        if n % 2 == 0:
            x[1, 0::2], x[1, 1::2] = -0.0, 0.0
    if n >= 8:
        x[0, n - 1], x[0, n // 2], x[2, n // 3] = -0.0, -np.inf, -np.inf
    R.assert_separated(x[0], "topk lattice row")
    return x, {k: R.topk(x, k)[0] for k in sorted({1, n, (n + 1) // 2})}


# --------------------------------------------------------------------------------------------------------------------- decode
DECODE_SHAPES = ((1, 1), (5, 5), (37, 20), (513, 512), (1023, 300), (1024, 512), (1024, 1))
DECODE_FLAT = ((37, 20), (1024, 512))
N2_JOIN = 48
N2_SIZES = (1, 255, 257)


def decode_case(A, K, mode="mixed"):
    rng = np.random.default_rng([3, A, K, mode == "flat"])
    bs = 2
    d = dict(cls=np.stack([class_rows(rng, A, mode) for _ in range(bs)]),
             quality=QUALITY[rng.integers(0, len(QUALITY), (bs, A, 2))], box=rng.standard_normal((bs, A, 11)).astype(np.float32),
             ids=(rng.integers(0, 5000, (bs, A)) + np.array(DECODE_ID_BASE)[:, None]).astype(np.int64),
             cls2d=np.stack([class_rows(rng, N2_JOIN) for _ in range(bs)]),
             box2d=rng.uniform(-0.2, 1.2, (bs, N2_JOIN, 4)).astype(np.float32), q2a=slot_anchors(rng, (bs, N2_JOIN), A),
             cam=rng.integers(-1, 6, N2_JOIN).astype(np.int32))
    if mode == "flat":
        d["quality"][:] = d["quality"][0, 0]
    for b in range(bs):     # slot 0 joins an anchor that is kept whatever K is: the best one of the first ranking
        d["q2a"][b, 0] = R.rank_desc(R.class_score(d["cls"][b])[0], 1)[0]
    d["ids"][rng.random((bs, A)) < 0.2] = -1
    return d


def decode_expected(d, K, with_quality, with_ids):
    want3 = R.decode3d(d["cls"], d["quality"] if with_quality else None, d["box"], d["ids"] if with_ids else None, K)
    for b in range(d["cls"].shape[0]):
        R.assert_separated(want3["score0"][b], "first ranking")
        R.assert_separated(want3["score"][b], "second ranking")
    want2 = R.decode2d(d["cls2d"], d["box2d"], d["q2a"], d["cam"], want3["rank_of_anchor"], CROP, RESIZE)
    return want3, want2


def slots_case(N2):
    rng = np.random.default_rng([5, N2])
    bs, A, K = 2, 37, 20
    d = dict(cls2d=np.stack([class_rows(rng, N2) for _ in range(bs)]), box2d=rng.uniform(-0.2, 1.2, (bs, N2, 4)).astype(np.float32),
             q2a=slot_anchors(rng, (bs, N2), A), cam=rng.integers(-1, 6, N2).astype(np.int32), rank=some_ranks(rng, bs, A, K))
    return d, R.decode2d(d["cls2d"], d["box2d"], d["q2a"], d["cam"], d["rank"], CROP, RESIZE)


def ragged_case(rows):
    """Three streams of rows + 1 (one slot more than the record has rows), 0 and rows - 1 slots, two cameras each."""
    rng = np.random.default_rng([6, rows])
    bs, A, K, cams = 3, 37, 20, 2
    counts = (rows + 1, 0, rows - 1)
    group_start, stream_of, cam_of = [0], [], []
    for b, n in enumerate(counts):
        for cam, m in enumerate((n // 2, n - n // 2)):
            group_start.append(group_start[-1] + m)
            stream_of += [b] * m
            cam_of += [b * cams + cam] * m
    S = group_start[-1]
    q2a = slot_anchors(rng, (S,), A) + np.asarray(stream_of, np.int32) * A      # flat anchors b * A + a ...
    q2a[3::5], q2a[4::7] = -1, bs * A                                          # ... and none at all
    d = dict(cls2d=class_rows(rng, S), box2d=rng.uniform(-0.2, 1.2, (S, 4)).astype(np.float32), q2a=q2a.astype(np.int32),
             cam=np.asarray(cam_of, np.int32), group_start=np.asarray(group_start, np.int32), rank=some_ranks(rng, bs, A, K),
             rows=rows, cams=cams, counts=counts)
    want = R.decode2d_ragged(d["cls2d"], d["box2d"], d["q2a"], d["cam"], d["group_start"], d["rank"], rows, cams, CROP, RESIZE)
    return d, want


# ----------------------------------------------------------------------------------------------------------------------- bank
GET_DT = (0.0, MAX_DT, -MAX_DT, float(np.nextafter(np.float32(MAX_DT), np.float32(np.inf))), -0.75)
UPDATE_SHAPES = ((2, 1), (37, 36), (37, 1), (1024, 600), (1023, 1))
COMMIT_SHAPES = ((5, 5), (37, 20), (1024, 1024), (1024, 600), (1023, 1))
COMMIT_COLD = ((5, 5), (1023, 1))      # these start without a previous confidence


def get_case():
    rng = np.random.default_rng(8)
    bs, n = len(GET_DT), 53                      # 265 rows: two workgroups
    d = dict(anchor=rng.standard_normal((bs, n, 11)).astype(np.float32), T=rng.standard_normal((bs, 4, 4)).astype(np.float32),
             dt=np.asarray(GET_DT, np.float32))
    return d, R.bank_get(d["anchor"], d["T"], d["dt"], MAX_DT, DEFAULT_DT)


def update_case(A, T):
    rng = np.random.default_rng([9, A, T])
    bs = 2
    cls = np.stack([class_rows(rng, A) for _ in range(bs)])
    if A >= 5:
        cls[0, 0] = (-0.0, -1.0, -2.5)           # a -0.0 maximum in front of the +0.0 maxima of the HALF rows: a tie
    d = dict(cls=cls, cur_f=rng.standard_normal((bs, A, E)).astype(np.float32), cur_a=rng.standard_normal((bs, A, 11)).astype(np.float32),
             cached_f=rng.standard_normal((bs, T, E)).astype(np.float32), cached_a=rng.standard_normal((bs, T, 11)).astype(np.float32),
             ids=(rng.integers(0, 5000, (bs, A)) + np.array(BANK_ID_BASE[:bs])[:, None]).astype(np.int64))
    return d


def update_expected(d, mask):
    want = R.bank_update(d["cls"], d["cur_f"], d["cur_a"], d["cached_f"], d["cached_a"], mask, d["ids"])
    for b in range(d["cls"].shape[0]):
        R.assert_separated(want["key"][b], "update ranking")
    return want


def lattice_confidence(rng, shape):
    """Lattice sigmoids times 0.6^j, j <= 3, rounded the way a commit rounds them (fp32 product per step)."""
    c = R.sigmoid(rng.integers(-20, 21, shape) * 0.25).astype(np.float32)
    for j in range(1, 4):
        c = np.where(rng.integers(0, 4, shape) >= j, c * np.float32(DECAY), c).astype(np.float32)
    return c


def commit_guard(out, threshold, active=None):
    for b in range(out["ranked"].shape[0]):
        if active is None or active[b]:
            R.assert_separated(out["ranked"][b], "commit ranking")
            if threshold is not None:
                R.assert_separated(np.append(out["fresh"][b], float(np.float32(threshold))), "id threshold")


def commit_case(bs, A, T, threshold, active=None, commits=3):
    """(initial state, frames, [(state, out) of the model after every commit], has_prev of the first commit)."""
    rng = np.random.default_rng([10, bs, A, T])
    ids = np.full((bs, A), -1, np.int64)
    ids[:, :T] = rng.integers(0, 5000, (bs, T)) + np.array(BANK_ID_BASE[:bs])[:, None]
    ids[:, :T][rng.random((bs, T)) < 0.4] = -1
    state = dict(conf=lattice_confidence(rng, (bs, T)), feature=rng.standard_normal((bs, T, E)).astype(np.float32),
                 anchor=rng.standard_normal((bs, T, 11)).astype(np.float32), ids=ids, prev_id=PREV_ID)
    state["conf"][:, T - 1] = np.float32(R.sigmoid(5.0))    # the last tracked row is confident: 0.6 of it beats every dim row
    frames = [dict(cls=np.stack([class_rows(rng, A, dim=0.7) for _ in range(bs)]), feature=rng.standard_normal((bs, A, E)).astype(np.float32),
                   anchor=rng.standard_normal((bs, A, 11)).astype(np.float32)) for _ in range(commits)]
    has_prev0 = (A, T) not in COMMIT_COLD
    want, st = [], state
    for f, fr in enumerate(frames):
        st, out = R.bank_commit(st, fr["cls"], fr["feature"], fr["anchor"], has_prev0 or f > 0, threshold, active, DECAY)
        commit_guard(out, threshold, active)
        want.append((st, out))
    return state, frames, want, has_prev0


STREAM = dict(bs=2, A=37, T=20, frames=3)


def stream_case(tie_free=False):
    """Three frames of two streams for InstanceBank: stream 1 is stale on frame 1 (|dt| > MAX_DT), stream 0 has dt = 0 on
    frame 2. tie_free: every row maximum of a frame is another lattice point (for a comparison with torch.topk)."""
    rng = np.random.default_rng([11, tie_free])
    bs, A = STREAM["bs"], STREAM["A"]

    def rows():
        if not tie_free:
            return np.stack([class_rows(rng, A, dim=0.7) for _ in range(bs)])
        top = np.stack([rng.permutation(41)[:A] - 20 for _ in range(bs)]) * 0.25
        rest = top[..., None] - rng.integers(1, 9, (bs, A, C - 1)) * 0.25
        return np.concatenate([rest[..., :1], top[..., None], rest[..., 1:]], -1).astype(np.float32)

    frames = []
    for f in range(STREAM["frames"]):
        Tm = np.tile(np.eye(4, dtype=np.float32), (bs, 1, 1))
        ang = rng.standard_normal(bs) * 0.2
        Tm[:, 0, 0], Tm[:, 0, 1], Tm[:, 1, 0], Tm[:, 1, 1] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
        Tm[:, :3, 3] = rng.standard_normal((bs, 3))
        dt = np.asarray([(0.5, 0.5), (0.5, 3.0), (0.0, -0.75)][f], np.float32)
        frames.append(dict(T=Tm, dt=dt, cls1=rows(), feat1=rng.standard_normal((bs, A, E)).astype(np.float32),
                           anchor1=rng.standard_normal((bs, A, 11)).astype(np.float32), cls2=rows(),
                           feat2=rng.standard_normal((bs, A, E)).astype(np.float32),
                           anchor2=rng.standard_normal((bs, A, 11)).astype(np.float32)))
    return frames


class StreamModel:
    """get -> update -> commit of rank_ref on one state, frame by frame (what InstanceBank does with its persistent state)."""

    def __init__(self, threshold):
        bs, A, T = STREAM["bs"], STREAM["A"], STREAM["T"]
        self.threshold, self.warm = threshold, False
        self.state = dict(conf=np.zeros((bs, T), np.float32), feature=np.zeros((bs, T, E), np.float32),
                          anchor=np.zeros((bs, T, 11), np.float32), ids=np.full((bs, A), -1, np.int64), prev_id=PREV_ID)

    def get(self, fr):
        return R.bank_get(self.state["anchor"], fr["T"], fr["dt"], MAX_DT, DEFAULT_DT) if self.warm else None

    def update(self, fr, got, warped):
        """warped f32: the cached anchors as get() delivered them (the merge copies them; it does not compute)."""
        if got is None:
            return None
        want = update_expected(dict(cls=fr["cls1"], cur_f=fr["feat1"], cur_a=fr["anchor1"], cached_f=self.state["feature"],
                                    cached_a=warped, ids=self.state["ids"]), got["mask"])
        self.state["ids"] = want["ids"]
        return want

    def commit(self, fr):
        self.state, out = R.bank_commit(self.state, fr["cls2"], fr["feat2"], fr["anchor2"], self.warm, self.threshold, None, DECAY)
        commit_guard(out, self.threshold)
        self.warm = True
        return out


# ================================================================================================================= the device
PAD = 256
SENTINEL = {torch.float32: -6.02e23, torch.int32: -77777, torch.int64: -77777, torch.uint8: 0xAB, torch.bool: True}


class Buffers:
    """Device buffers inside sentinel-filled ones; check() after the launches."""

    def __init__(self):
        self.all = []

    def new(self, shape, dtype=torch.float32, init=None):
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape, dtype=np.int64))
        whole = torch.full((n + 2 * PAD,), SENTINEL[dtype], dtype=dtype, device="cuda")
        inner = whole[PAD:PAD + n].view(shape)
        if init is not None:
            inner.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype))
        self.all.append((whole, n))
        return inner

    def check(self):
        torch.cuda.synchronize()
        assert self.all
        for whole, n in self.all:
            s = SENTINEL[whole.dtype]
            assert bool((whole[:PAD] == s).all()) and bool((whole[PAD + n:] == s).all()), "write outside an output"


def api():
    from simpb_amd import _lib as L
    from simpb_amd.plugin.ops import _ptr, _stream
    return L, L.lib(), _ptr, _stream


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize])


def assert_scores(name, got, want):
    """got fp32 within SCORE_BOUND of the float64 model, relative (a model value of exactly 0 allows nothing)."""
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ulps = np.where(want != 0, err / (np.abs(want) * R.ULP), np.where(err == 0, 0.0, np.inf))
    note(f"{name} ulp", float(ulps.max()) if ulps.size else 0.0)
    assert (err <= SCORE_BOUND * np.abs(want)).all(), (name, float(ulps.max()))


def assert_close(name, got, want, bound):
    err = float(np.abs(got.astype(np.float64) - want).max()) if got.size else 0.0
    note(f"{name} abs", err)
    assert err <= bound, (name, err, bound)


# ---------------------------------------------------------------------------------------------------------------------- top-k
@gpu
@pytest.mark.parametrize("n", TOPK_N)
def test_topk_rows_indices_are_the_models_and_values_the_inputs_own_bits(n):
    L, lib, P, S = api()
    x, want = topk_case(n)
    xd = dev(x)
    for k, index in want.items():
        B = Buffers()
        val, idx = B.new((3, k)), B.new((3, k), torch.int32)
        L.check(lib.simpb_topk_rows(P(val), P(idx), P(xd), 3, n, k, S()), "simpb_topk_rows")
        B.check()
        assert np.array_equal(host(idx), index), (n, k)
        assert np.array_equal(bits(host(val)), bits(np.take_along_axis(x, index, 1))), (n, k)   # -0.0 stays -0.0


# --------------------------------------------------------------------------------------------------------------------- decode
def run_decode3d(d, K, with_quality, with_ids, B):
    L, lib, P, S = api()
    bs, A, _ = d["cls"].shape
    rec, rank = B.new((bs, K, 15)), B.new((bs, A), torch.int32)
    quality, ids = dev(d["quality"]) if with_quality else None, dev(d["ids"]) if with_ids else None
    cls, box = dev(d["cls"]), dev(d["box"])
    L.check(lib.simpb_decode3d_record(P(rec), P(rank), P(cls), P(quality) if with_quality else None, P(box),
                                      P(ids) if with_ids else None, bs, A, C, K, S()), "simpb_decode3d_record")
    return rec, rank


def run_decode2d(d, rank, B):
    L, lib, P, S = api()
    bs, N2, _ = d["cls2d"].shape
    rec = B.new((bs, N2, 8))
    ins = [dev(d[k]) for k in ("cls2d", "box2d", "q2a", "cam")]
    L.check(lib.simpb_decode2d_record(P(rec), *[P(t) for t in ins], P(rank), bs, N2, C, rank.shape[1], float(CROP[2] - CROP[0]),
                                      float(CROP[3] - CROP[1]), float(CROP[1]), RESIZE, S()), "simpb_decode2d_record")
    return rec


def check_rec3d(got, rank, want, with_quality):
    assert np.array_equal(rank, want["rank_of_anchor"])                 # which anchor sits in which row; no row without one
    assert np.array_equal(got[..., 11], want["label"].astype(np.float32))
    assert np.array_equal(bits(got[..., 13:15]), bits(want["lanes"].view(np.int32)))
    assert np.array_equal(bits(got[..., [0, 1, 2, 7, 8, 9]]), bits(want["raw_box"][..., [0, 1, 2, 8, 9, 10]]))
    assert_scores("decode3d score", got[..., 10], want["score"])
    assert_scores("decode3d column 12", got[..., 12], want["column12"])  # (distinct first scores are >= 1.9e-3 apart: the position)
    if not with_quality:
        assert np.array_equal(bits(got[..., 12]), bits(got[..., 10]))
    assert (np.diff(got[..., 10].astype(np.float64), axis=1) <= 0).all()
    assert_close("decode3d exp columns", got[..., 3:6], want["box"][..., 3:6], EXP_BOUND)
    assert_close("decode3d atan2 column", got[..., 6], want["box"][..., 6], ATAN2_BOUND)


def check_rec2d(name, got, want):
    assert np.array_equal(got[..., 5:8], want[..., 5:8].astype(np.float32))    # label, rank of the slot's anchor, camera
    assert_scores(name + " score", got[..., 4], want[..., 4])
    assert_close(name + " pixel columns", got[..., 0:4], want[..., 0:4], PIXEL_BOUND)


@gpu
@pytest.mark.parametrize("with_ids", [True, False], ids=["ids", "no_ids"])
@pytest.mark.parametrize("with_quality", [True, False], ids=["quality", "no_quality"])
@pytest.mark.parametrize("A,K", DECODE_SHAPES)
def test_decode3d_record_and_the_2d_join(A, K, with_quality, with_ids):
    d = decode_case(A, K)
    want3, want2 = decode_expected(d, K, with_quality, with_ids)
    B = Buffers()
    rec3d, rank = run_decode3d(d, K, with_quality, with_ids, B)
    rec2d = run_decode2d(d, rank, B)
    B.check()
    check_rec3d(host(rec3d), host(rank), want3, with_quality)
    check_rec2d("decode2d join", host(rec2d), want2)


@gpu
@pytest.mark.parametrize("A,K", DECODE_FLAT)
def test_decode3d_with_all_scores_equal_keeps_the_anchor_order(A, K):
    d = decode_case(A, K, "flat")
    want3, want2 = decode_expected(d, K, True, True)
    assert np.array_equal(want3["anchor"], np.tile(np.arange(K), (2, 1)))
    B = Buffers()
    rec3d, rank = run_decode3d(d, K, True, True, B)
    rec2d = run_decode2d(d, rank, B)
    B.check()
    check_rec3d(host(rec3d), host(rank), want3, True)
    check_rec2d("decode2d join", host(rec2d), want2)


@gpu
@pytest.mark.parametrize("N2", N2_SIZES)
def test_decode2d_record(N2):
    d, want = slots_case(N2)
    B = Buffers()
    rec = run_decode2d(d, dev(d["rank"]), B)
    B.check()
    check_rec2d("decode2d", host(rec), want)


@gpu
@pytest.mark.parametrize("rows", N2_SIZES)
def test_decode2d_ragged_record(rows):
    L, lib, P, S = api()
    d, want = ragged_case(rows)
    B = Buffers()
    rec = B.new((3, rows, 8))
    ins = [dev(d[k]) for k in ("cls2d", "box2d", "q2a", "cam", "group_start", "rank")]
    L.check(lib.simpb_decode2d_record_ragged(P(rec), *[P(t) for t in ins], 3, rows, d["cams"], C, d["rank"].shape[1],
                                             float(CROP[2] - CROP[0]), float(CROP[3] - CROP[1]), float(CROP[1]), RESIZE, S()),
            "simpb_decode2d_record_ragged")
    B.check()
    got = host(rec)
    check_rec2d("decode2d ragged", got, want)
    for b, n in enumerate(d["counts"]):      # pad rows exactly: zeros, rank -1, camera -1
        assert np.array_equal(got[b, min(n, rows):], want[b, min(n, rows):].astype(np.float32)), b


# ----------------------------------------------------------------------------------------------------------------------- bank
@gpu
def test_bank_get_mask_time_step_and_warp():
    L, lib, P, S = api()
    d, want = get_case()
    bs, n, _ = d["anchor"].shape
    B = Buffers()
    out, mask, dt_out = B.new((bs, n, 11)), B.new((bs,), torch.uint8), B.new((bs,))
    ins = [dev(d[k]) for k in ("anchor", "T", "dt")]
    L.check(lib.simpb_bank_get(P(out), P(mask), P(dt_out), *[P(t) for t in ins], bs, n, MAX_DT, DEFAULT_DT, S()), "simpb_bank_get")
    B.check()
    assert host(mask).tolist() == want["mask"].astype(int).tolist() == [1, 1, 1, 0, 1]
    assert np.array_equal(bits(host(dt_out)), bits(want["dt"])) and want["dt"].tolist() == [0.5, 2.0, -2.0, 0.5, -0.75]
    check_warp(host(out), d["anchor"], want)


def check_warp(got, stored, want):
    assert np.array_equal(bits(got[..., 3:6]), bits(stored[..., 3:6]))
    err = np.abs(got.astype(np.float64) - want["anchor"])
    moved = [0, 1, 2, 6, 7, 8, 9, 10]
    note("bank_get warp / (2^-24 * size)", float((err[..., moved] / (want["size"][..., moved] * 2.0 ** -24)).max()))
    assert (err[..., moved] <= WARP_BOUND * want["size"][..., moved]).all()


@gpu
@pytest.mark.parametrize("mask", [(1, 0), (0, 1)], ids=["10", "01"])
@pytest.mark.parametrize("A,T", UPDATE_SHAPES)
def test_bank_update_rank_and_merge(A, T, mask):
    L, lib, P, S = api()
    d = update_case(A, T)
    want = update_expected(d, mask)
    B = Buffers()
    index, out_f, out_a = B.new((2, A - T), torch.int32), B.new((2, A, E)), B.new((2, A, 11))
    ids = B.new((2, A), torch.int64, d["ids"])
    t = {k: dev(d[k]) for k in ("cls", "cur_f", "cur_a", "cached_f", "cached_a")}
    md = dev(np.asarray(mask, np.uint8))
    L.check(lib.simpb_bank_update_rank(P(index), P(t["cls"]), 2, A, C, T, S()), "simpb_bank_update_rank")
    L.check(lib.simpb_bank_update_merge(P(out_f), P(out_a), None, P(ids), P(index), P(t["cur_f"]), P(t["cur_a"]), None,
                                        P(t["cached_f"]), P(t["cached_a"]), None, P(md), None, 0, None, 2, A, T, E, 0, S()),
            "simpb_bank_update_merge")
    B.check()
    assert np.array_equal(host(index), want["index"])
    assert np.array_equal(bits(host(out_f)), bits(want["feature"])) and np.array_equal(bits(host(out_a)), bits(want["anchor"]))
    assert np.array_equal(host(ids), want["ids"])


def run_commits(kind, state, frames, has_prev0, threshold, active, B):
    """The commits back to back on one device state; returns what every commit left (host copies)."""
    L, lib, P, S = api()
    bs, A = state["ids"].shape
    T = state["conf"].shape[1]
    st = dict(conf=B.new((bs, T), init=state["conf"]), feature=B.new((bs, T, E), init=state["feature"]),
              anchor=B.new((bs, T, 11), init=state["anchor"]), ids=B.new((bs, A), torch.int64, state["ids"]),
              prev=B.new((1,), torch.int64, np.asarray([state["prev_id"]], np.int64)))
    sync = B.new((2,), torch.int32, np.zeros(2, np.int32)) if kind == "streams" else None
    act = dev(np.asarray(active, np.uint8)) if active is not None else None
    left = []
    for f, fr in enumerate(frames):
        ids_out, scratch = B.new((bs, A), torch.int64), B.new((bs, T), torch.int32)
        ins = [dev(fr[k]) for k in ("feature", "anchor", "cls")]
        args = [P(st["conf"]), P(st["feature"]), P(st["anchor"]), P(st["ids"]), P(st["prev"]), P(ids_out), P(scratch),
                *[P(t) for t in ins], bs, A, C, T, E, 1 if (has_prev0 or f) else 0, DECAY, 0 if threshold is None else 1,
                0.0 if threshold is None else threshold, None, 0, None]
        if active is not None:
            status = lib.simpb_bank_cache_streams_active(*args, P(sync) if sync is not None else None, P(act), S())
        elif kind == "streams":
            status = lib.simpb_bank_cache_streams(*args, P(sync), S())
        else:
            status = lib.simpb_bank_cache(*args, S())
        L.check(status, "simpb_bank_cache")
        torch.cuda.synchronize()
        left.append({k: host(v).copy() for k, v in dict(st, ids_out=ids_out, index=scratch).items()})
    B.check()
    return left


def check_commits(left, want, active=None):
    for f, (got, (state, out)) in enumerate(zip(left, want)):
        live = [b for b in range(out["ids"].shape[0]) if active is None or active[b]]
        assert np.array_equal(got["index"][live], out["index"][live]), f
        assert int(got["index"][live].max()) < out["ids"].shape[1]
        assert np.array_equal(got["ids_out"], out["ids"]), f
        assert np.array_equal(got["ids"], state["ids"]) and int(got["prev"][0]) == state["prev_id"], f
        assert np.array_equal(bits(got["feature"]), bits(state["feature"])) and np.array_equal(bits(got["anchor"]), bits(state["anchor"])), f
        assert_scores(f"commit {f} kept confidence", got["conf"][live], out["kept"][live])
        for b in set(range(out["ids"].shape[0])) - set(live):     # a paused stream: its rows as they were
            assert np.array_equal(bits(got["conf"][b]), bits(state["conf"][b])), (f, b)


@gpu
@pytest.mark.parametrize("threshold", [None, THRESHOLD], ids=["no_threshold", "threshold"])
@pytest.mark.parametrize("kind", ["serial", "streams"])
@pytest.mark.parametrize("A,T", COMMIT_SHAPES)
@pytest.mark.parametrize("bs", [1, 2, 3])
def test_bank_commit_three_times_on_the_state_it_left(bs, A, T, kind, threshold):
    state, frames, want, has_prev0 = commit_case(bs, A, T, threshold)
    left = run_commits(kind, state, frames, has_prev0, threshold, None, Buffers())
    check_commits(left, want)


@gpu
@pytest.mark.parametrize("kind", ["serial", "streams"])
def test_bank_commit_with_a_paused_stream(kind):
    active = (1, 0, 1)
    state, frames, want, has_prev0 = commit_case(3, 37, 20, THRESHOLD, active)
    left = run_commits(kind, state, frames, has_prev0, THRESHOLD, active, Buffers())
    check_commits(left, want, active)


# ---------------------------------------------------------------------------------------------------- InstanceBank, three frames
class GuardedTorch:
    """Stands in for `torch` inside plugin/instance_bank.py: what the bank allocates lies inside sentinel-filled buffers."""

    def __init__(self, buffers):
        self.buffers = buffers

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=None, device=None):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        return self.buffers.new(shape, dtype or torch.float32)

    def zeros(self, *shape, **kw):
        return self.empty(*shape, **kw).zero_()

    def full(self, shape, value, **kw):
        return self.empty(shape, **kw).fill_(value)

    def empty_like(self, t):
        return self.buffers.new(t.shape, t.dtype)


def make_bank(device):
    from simpb_amd import synth
    from simpb_amd.plugin import instance_bank as ib
    bank = ib.InstanceBank(num_anchor=STREAM["A"], embed_dims=E, anchor=synth.anchors(STREAM["A"]), num_temp_instances=STREAM["T"],
                           anchor_handler=dict(type="SparseBox3DKeyPointsGenerator"), confidence_decay=DECAY, feat_grad=False,
                           max_time_interval=MAX_DT, default_time_interval=DEFAULT_DT)
    return bank.to(device).eval()


def run_bank_frame(bank, f, fr, threshold, fused):
    """One frame through InstanceBank: (dt, mask, warped cached anchors, merged feature, merged anchor, ids)."""
    bs = STREAM["bs"]
    t = {k: torch.from_numpy(v).to(bank.anchor.device) for k, v in fr.items()}
    _, _, _, ca, dt = bank.get(bs, {"bank_inputs": (t["T"], t["dt"])} if f else {})
    if f == 0:
        bank.prev_id.fill_(PREV_ID)      # (get() on a cold bank has just reset the state)
    mask = bank.mask
    feat, anc = bank.update(t["feat1"], t["anchor1"], t["cls1"])
    ids = bank.cache_and_assign_ids(t["feat2"], t["anchor2"], t["cls2"], metas={}, threshold=threshold) if fused else None
    if ids is None:
        assert not fused
        bank.cache(t["feat2"], t["anchor2"], t["cls2"], metas={})
        ids = bank.get_instance_id(t["cls2"], t["anchor2"], threshold)
    return dt, mask, ca, feat, anc, ids


@gpu
def test_instance_bank_stream_with_a_threshold_follows_the_model_frame_by_frame():
    from simpb_amd.plugin import instance_bank as ib, routes
    frames, model = stream_case(), StreamModel(THRESHOLD)
    B = Buffers()
    bank = make_bank("cuda")
    real, ib.torch = ib.torch, GuardedTorch(B)
    try:
        bank.enable_static(STREAM["bs"], torch.device("cuda"))
        with routes.override(fused_bank=True), torch.no_grad():
            for f, fr in enumerate(frames):
                want_get = model.get(fr)
                dt, mask, ca, feat, anc, ids = run_bank_frame(bank, f, fr, THRESHOLD, True)
                if want_get is None:
                    assert ca is None and dt.tolist() == [DEFAULT_DT] * STREAM["bs"]
                    assert np.array_equal(bits(host(feat)), bits(fr["feat1"])) and np.array_equal(bits(host(anc)), bits(fr["anchor1"]))
                else:
                    assert host(mask).tolist() == want_get["mask"].tolist() and np.array_equal(bits(host(dt)), bits(want_get["dt"]))
                    check_warp(host(ca), model.state["anchor"], want_get)
                    want = model.update(fr, want_get, host(ca))
                    assert np.array_equal(bits(host(feat)), bits(want["feature"])), f
                    assert np.array_equal(bits(host(anc)), bits(want["anchor"])), f
                out = model.commit(fr)
                st = model.state
                assert np.array_equal(host(ids), out["ids"]), f
                assert np.array_equal(host(bank.instance_id), st["ids"]) and int(bank.prev_id) == st["prev_id"], f
                assert np.array_equal(bits(host(bank.cached_feature)), bits(st["feature"])), f
                assert np.array_equal(bits(host(bank.cached_anchor)), bits(st["anchor"])), f
                assert_scores(f"bank frame {f} confidence", host(bank.confidence), out["kept"])
    finally:
        ib.torch = real
    B.check()


# --------------------------------------------------------------------------------------------------------- entry-point refusals
def test_entry_points_refuse_what_the_kernels_cannot_hold():
    """Every one of these returns before any launch (no device is touched): SIMPB_EINVAL."""
    from simpb_amd import _lib, build
    build.build_extension()
    h = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    P = lambda n: [one] * n   # noqa: E731
    EINVAL = 1   # include/simpb_hip.h SIMPB_EINVAL
    assert h.simpb_topk_rows(*P(3), 1, 2049, 1, null) == EINVAL                                   # n = 2049
    assert h.simpb_topk_rows(*P(3), 1, 5, 6, null) == EINVAL                                      # k > n
    assert h.simpb_decode3d_record(*P(6), 1, 1025, C, 1, null) == EINVAL                          # A = 1025
    assert h.simpb_decode3d_record(*P(6), 1, 1024, C, 513, null) == EINVAL                        # K = 513
    assert h.simpb_decode3d_record(*P(6), 1, 5, C, 6, null) == EINVAL                             # K > A
    assert h.simpb_bank_update_rank(*P(2), 1, 37, C, 37, null) == EINVAL                          # T = A
    assert h.simpb_bank_update_merge(*P(13), 0, null, 1, 37, 37, E, 0, null) == EINVAL            # T = A
    assert h.simpb_bank_update_merge(*P(13), 0, null, 1, 37, 20, 6, 0, null) == EINVAL            # E % 4
    assert h.simpb_bank_update(*P(10), 1, 37, C, 37, E, null) == EINVAL                           # T = A
    for entry, tail in ((h.simpb_bank_cache, [null]), (h.simpb_bank_cache_streams, [one, null]),
                        (h.simpb_bank_cache_streams_active, [one, one, null])):
        assert entry(*P(10), 2, 37, C, 38, E, 1, DECAY, 0, 0.0, null, 0, null, *tail) == EINVAL   # T > A
        assert entry(*P(10), 2, 37, C, 20, 6, 1, DECAY, 0, 0.0, null, 0, null, *tail) == EINVAL   # E % 4
        assert entry(*P(10), 2, 1025, C, 20, E, 1, DECAY, 0, 0.0, null, 0, null, *tail) == EINVAL  # A = 1025
