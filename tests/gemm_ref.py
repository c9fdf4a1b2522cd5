"""Float64 model of csrc/gemm.hip (grouped, segment-input GEMM; segmented LayerNorm), csrc/linear.hip and the row dot of
csrc/rowops.hip, the Python twin of the kernel selection in simpb_gemm_f32, and the inputs, buffers and case tables of
tests/test_gemm_float64.py. Nothing here needs a GPU: tests/test_gemm_ref_host.py proves the models against torch's float64
operators, the routes and edges of the tables, and that a plain float32 evaluation stays under half of every bound.

Bounds (tests/test_split_range.py, tests/test_mlp_chain_float64.py; no constants of its own):
  (b) per element |got - want| <= 2e-5 * (|x| . |W|^T + |bias| + flag |bias2|), no absolute floor;
  (c) on the split routes max err <= 4 * e_exact + 1e-7 * max magnitude, e_exact the exact-fp32 kernel's error;
  (d) one-hot x on an exact route: float32(W[n, k(r)]) + float32(bias[n]) under torch.equal; on a split route
      2^-21 of the row's largest |w|;
  LayerNorm absolute 2e-5 on well-conditioned rows, row dot absolute 1e-5."""
import collections
import itertools
import math

import numpy as np
import torch

from simpb_amd import synth
from simpb_amd.plugin import dense

REL = 2e-5            # bound (b)
LN_ABS = 2e-5         # tests/test_dense.py: LayerNorm on well-conditioned rows
ROWDOT_ABS = 1e-5     # tests/test_dense.py: row dot + sigmoid
PLACE_SPLIT = 2.0 ** -21   # (d) on split routes, and the half-pair word: two halfs carry 22 bits
HALF_MIN_NORMAL = 2.0 ** -14
SENTINEL = -777.25    # exactly representable; no kernel output of these inputs comes near it
LN_EPS = 1e-5


# ------------------------------------------------------------------------------------------------ float64 models
def products(x, w):
    """(x . W^T, |x| . |W|^T) in float64: the part of gemm_ref that a sweep over slices of x and W computes once."""
    x, w = x.double(), w.double()
    return x @ w.t(), x.abs() @ w.abs().t()


def gemm_ref(xs, w, bias=None, relu=False, live=None, row_flag=None, bias2=None, product=None):
    """(y, magnitude), float64 [M, N]: y = relu?([x0 | x1 | ...] . W^T + bias + row_flag * bias2) with rows >= min(M, live)
    zeros; magnitude = |x| . |W|^T + |bias| + flag * |bias2| (rows past live: 0). Rows past live are never read: they may
    hold NaN. `product`: products() of these operands (or the matching slice of a larger pair's), to share among cases."""
    m = xs[0].shape[0]
    live = m if live is None else max(0, min(m, int(live)))
    if product is None:
        x = torch.cat([t.double() for t in xs], -1).clone()
        x[live:] = 0
        product = products(x, w)
    y, mag = product[0].clone(), product[1].clone()
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    if row_flag is not None:
        f = (row_flag != 0).double()[:, None]
        y, mag = y + f * bias2.double(), mag + f * bias2.double().abs()
    if relu:
        y = y.clamp_min(0)
    y[live:] = 0
    mag[live:] = 0
    return y, mag


def halfs_of(y):
    """(hi, lo) halfs of the float32 tensor y as out_fmt = 1 stores them (hi in the low 16 bits of the word, lo above):
    hi = half(y), lo = half((y - hi) * 2048), both round-to-nearest-even."""
    y = y.float()
    hi = y.half()
    lo = ((y - hi.float()) * 2048.0).half()
    return hi, lo


def halfs_word(y):
    hi, lo = halfs_of(y)
    return (hi.view(torch.int16).to(torch.int32) & 0xFFFF) | (lo.view(torch.int16).to(torch.int32) << 16)


def halfs_value(word):
    """Inverse: the float64 value hi + lo / 2048 of int32 words."""
    word = word.to(torch.int32)
    hi = (word & 0xFFFF).to(torch.int16).view(torch.float16)
    lo = ((word >> 16) & 0xFFFF).to(torch.int16).view(torch.float16)
    return hi.double() + lo.double() / 2048.0


def layernorm_ref(xs, gamma, beta, live=None):
    """(y, magnitude): LayerNorm over cat(xs), eps 1e-5, biased variance, float64; rows >= live zeros."""
    x = torch.cat([t.double() for t in xs], -1)
    m = x.shape[0]
    live = m if live is None else max(0, min(m, int(live)))
    x = x.clone()
    x[live:] = 0
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    xhat = (x - mean) / torch.sqrt(var + LN_EPS)
    y = xhat * gamma.double() + beta.double()
    mag = xhat.abs() * gamma.double().abs() + beta.double().abs()
    y[live:] = 0
    mag[live:] = 0
    return y, mag


def layernorm_f32(xs, gamma, beta):
    """The same formula evaluated in float32 on the CPU, every operation rounded once: what e32 of bound (c) measures."""
    x = torch.cat([t.float() for t in xs], -1)
    mean = x.sum(-1, keepdim=True) / x.shape[-1]
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / x.shape[-1]
    return d * (1.0 / torch.sqrt(var + torch.tensor(LN_EPS, dtype=torch.float32))) * gamma.float() + beta.float()


def rowdot_sigmoid_ref(x, w, b, live=None):
    m = x.shape[0]
    live = m if live is None else max(0, min(m, int(live)))
    x = x.double().clone()
    x[live:] = 0
    y = torch.sigmoid(x @ w.double().reshape(-1) + (b.double() if b is not None else 0.0))
    y[live:] = 0
    return y[:, None]


# ------------------------------------------------------------------------------------------------ the route rule
Route = collections.namedtuple("Route", "name kernel tile_m tile_n depth chunk split")
ROUTES = {r.name: r for r in (
    Route("f32_d4k64", "gemm_f32_kernel<32, 4, 64>", 32, 32, 4, 64, False),
    Route("f32_d2k128", "gemm_f32_kernel<32, 2, 128>", 32, 32, 2, 128, False),
    Route("f32_n64", "gemm_f32_kernel<64, 2, 64>", 32, 64, 2, 64, False),
    Route("f16_d2k128", "gemm_f16x3_kernel<32, 2, 128>", 32, 32, 2, 128, True),
    Route("f16_n64", "gemm_f16x3_kernel<64, 2, 64>", 32, 64, 2, 64, True),
    Route("f16_wide", "gemm_f16x3_wide_kernel<2>", 64, 128, 2, 64, True),
)}
SPLIT_ROUTES = tuple(n for n, r in ROUTES.items() if r.split)
EXACT_ROUTES = tuple(n for n, r in ROUTES.items() if not r.split)
NARROW_MIN_TILES, WIDE_MIN_TILES = 200, 400   # csrc/gemm.hip: bn, kWideMinTiles


def tiles(jobs, tm, tn):
    return sum(-(-j["M"] // tm) * -(-j["N"] // tn) for j in jobs)


def in_window(w):
    """dense.split_in_window without its warning: every row's largest |w| in SPLIT_WINDOW, or the row all zeros."""
    m = w.detach().double().abs().amax(-1)
    lo, hi = dense.SPLIT_WINDOW
    return bool(torch.isfinite(m).all()) and bool(((m == 0) | ((m >= lo) & (m < hi))).all())


def route_of(jobs, split=True):
    """The instantiation simpb_gemm_f32 launches for `jobs` (dicts with M, N, segs and, optionally, w_contiguous and
    w_in_window, both True when absent) with routes.gemm_split_fp16 = split: the rule of csrc/gemm.hip's entry point and of
    plugin/dense.py gemm() restated. One launch takes one kernel: a single job off the split route takes them all off."""
    on_split = split and all(j.get("w_contiguous", True) and j.get("w_in_window", True) and
                             all(k % 128 == 0 for k in j["segs"]) for j in jobs)
    wide_k = all(k % 128 == 0 for j in jobs for k in j["segs"]) and all(sum(j["segs"]) >= 512 for j in jobs)
    bn = 64 if tiles(jobs, 32, 64) >= NARROW_MIN_TILES else 32
    if on_split and tiles(jobs, 64, 128) >= WIDE_MIN_TILES:
        return ROUTES["f16_wide"]
    if on_split:
        return ROUTES["f16_n64" if bn == 64 else "f16_d2k128"]
    if bn == 64:
        return ROUTES["f32_n64"]
    return ROUTES["f32_d2k128" if wide_k else "f32_d4k64"]


def total_tiles(jobs, split=True):
    r = route_of(jobs, split)
    return tiles(jobs, r.tile_m, r.tile_n)


# ------------------------------------------------------------------------------------------------ case tables
# Per route: the M and N of the tile sweep (one below / at / one above a tile border and a partial tile of 32 + 1, placed
# so that the tile thresholds 200 and 400 hold at every pair), the segments of the sweep (a chunk count with a loop tail
# where the route admits one), the ragged shape of the other groups (three or more row tiles) and the chunk counts.
_SMALL = (1, 31, 32, 33, 63, 65)
SWEEP = {
    "f32_d4k64": dict(ms=_SMALL, ns=_SMALL, segs=(64, 256), ragged=(70, 65), chunks=tuple(range(1, 10))),
    "f32_d2k128": dict(ms=_SMALL, ns=_SMALL, segs=(128, 512), ragged=(70, 65), chunks=(4, 5, 6, 7)),
    "f32_n64": dict(ms=(319, 320, 321), ns=(1279, 1280, 1281, 1313), segs=(64, 128), ragged=(321, 1313), chunks=(1, 2, 3, 4, 5)),
    "f16_d2k128": dict(ms=_SMALL, ns=_SMALL, segs=(128, 256), ragged=(70, 65), chunks=(1, 2, 3, 4, 5)),
    "f16_n64": dict(ms=(319, 320, 321), ns=(1279, 1280, 1281, 1313), segs=(128, 128), ragged=(321, 1313), chunks=(2, 4, 6)),
    "f16_wide": dict(ms=(1279, 1280, 1281, 1313), ns=(2559, 2560, 2561, 2593), segs=(128,), ragged=(1281, 2561), chunks=(2, 4, 6)),
}
# what the issue asks of each table (asserted by the host test, so an edit cannot thin them)
REQUIRED_CHUNKS = {"f32_d4k64": range(1, 10), "f32_d2k128": (4, 5, 6, 7), "f32_n64": (1, 2, 3, 4, 5),
                   "f16_d2k128": (1, 2, 3, 4, 5), "f16_n64": (2, 4, 6), "f16_wide": (2, 4, 6)}


def chunk_segs(route, count):
    """Segments that give `count` chunks on `route`: one segment, but for the depth-4 kernel a leading 64-wide one, which
    keeps K >= 512 off the 128-deep kernel."""
    k = ROUTES[route].chunk * count
    if route == "f32_d4k64" and count > 1:
        return (64, k - 64)
    return (k,)


def job_dims(m, n, segs):
    return dict(M=m, N=n, segs=tuple(segs))


def exact_split(route):
    """The routes.gemm_split_fp16 value a case of `route` runs under."""
    return ROUTES[route].split


def sweep_cases(route):
    """[(M, N, segs, bias, relu)] of the tile sweep: the M x N set at one K, bias and relu cycling through their four forms."""
    t = SWEEP[route]
    forms = list(itertools.product((True, False), (False, True)))
    return [(m, n, t["segs"], *forms[i % 4]) for i, (m, n) in enumerate(itertools.product(t["ms"], t["ns"]))]


def chunk_cases(route):
    t = SWEEP[route]
    forms = list(itertools.product((True, False), (False, True)))
    return [(*t["ragged"], chunk_segs(route, c), *forms[i % 4]) for i, c in enumerate(t["chunks"])]


def compositions(total, unit, max_parts=4):
    """Every ordered way to write `total` as 1..max_parts multiples of `unit`."""
    n = total // unit
    out = []
    for parts in range(1, max_parts + 1):
        for cuts in itertools.combinations(range(1, n), parts - 1):
            edges = (0,) + cuts + (n,)
            out.append(tuple((b - a) * unit for a, b in zip(edges, edges[1:])))
    return out


SEGMENT_SHAPE = {"f32_d4k64": (33, 40), "f32_d2k128": (33, 40), "f32_n64": (321, 1281), "f16_d2k128": (33, 40),
                 "f16_n64": (321, 1281), "f16_wide": (1281, 2561)}


def segment_cases(route):
    """Compositions of K = 256 and K = 512 into 1-4 segments that the route admits: units of 64 on the depth-64 exact
    kernels (those with a segment that is no multiple of 128, which is what keeps a launch there; plus the all-128 ones
    below K = 512 for the depth-4 kernel), units of 128 elsewhere. Capped, where there are many, at a subset that still puts
    a boundary on every chunk index and holds every segment count."""
    r = ROUTES[route]
    m, n = SEGMENT_SHAPE[route]
    out = []
    for k in (256, 512):
        unit = 64 if route in ("f32_d4k64", "f32_n64") else 128
        comps = [c for c in compositions(k, unit) if route_of([job_dims(m, n, c)], r.split).name == route]
        if len(comps) > 12:
            keep, seen = [], set()
            for c in sorted(comps, key=lambda c: (-len(c), c)):
                cuts = set(itertools.accumulate(c[:-1]))
                if not cuts <= seen or len(c) not in {len(q) for q in keep}:
                    keep.append(c)
                    seen |= cuts
            comps = keep
        out += comps
    return out


def live_values(route):
    tm = ROUTES[route].tile_m
    m = SWEEP[route]["ragged"][0]
    return (0, 1, tm - 1, tm, tm + 1, m - 1, m, m + 5)


# Grouped launches. Per case a list of (M, N, segs, bias, relu, extra) with extra one of None, "capacity" (m_live = 0),
# "flags" (row_flag + bias2), "adjacent" (writes the column range next to the previous job's, same buffer).
GROUPED = {
    "total1": ("f32_d4k64", [(5, 20, (64,), True, False, None)]),
    "total7": ("f32_d4k64", [(33, 33, (64, 64), True, False, None), (70, 30, (192,), False, True, None)]),
    "total8": ("f32_d2k128", [(64, 64, (512,), True, False, None), (33, 32, (128, 384), True, True, None),
                              (31, 33, (640,), False, False, None)]),
    "total9": ("f16_d2k128", [(65, 33, (128,), True, False, None), (32, 32, (128, 128), False, False, "capacity"),
                              (17, 33, (256,), True, True, None)]),
    "four_jobs": ("f32_d4k64", [(31, 65, (64, 128), True, False, None), (96, 32, (64,), False, False, "capacity"),
                                     (70, 40, (128, 64), True, True, "flags"), (70, 24, (128, 64), True, False, "adjacent")]),
    "f16_adjacent": ("f16_d2k128", [(70, 40, (128, 128), True, False, None), (70, 24, (128, 128), True, True, "adjacent"),
                                         (7, 200, (384,), False, False, "flags")]),
    "n64_three_jobs": ("f32_n64", [(161, 1281, (64, 64), True, False, None), (20, 70, (128,), False, True, None),
                             (159, 1217, (192,), True, False, "flags")]),
    "f16_n64_capacity": ("f16_n64", [(161, 1281, (128,), True, False, None), (64, 64, (256,), False, False, "capacity"),
                                 (190, 1153, (128, 128), True, True, None)]),
    "wide_four_jobs": ("f16_wide", [(641, 1281, (128,), True, False, None), (705, 1281, (128, 128), False, True, None),
                                    (640, 1281, (256,), True, False, "flags"), (30, 5000, (128,), True, False, None)]),
}
REQUIRED_TOTALS = (1, 7, 8, 9)


def grouped_dims(case):
    return [job_dims(m, n, segs) for m, n, segs, *_ in GROUPED[case][1]]


LN_WIDTHS = ((64, 0), (256, 0), (512, 0), (256, 256), (64, 448), (320, 64))
LN_ROWS = (1, 3, 4, 5, 301)
LN_KINDS = ("randn", "offset", "const", "tiny")
ROWDOT_K = (4, 252, 256, 260, 512)
ROWDOT_ROWS = (1, 3, 4, 5, 301)
LINEAR_M, LINEAR_N, LINEAR_K = (1, 63, 64, 65, 129), (1, 255, 256, 257, 513), (32, 64, 96)


def rows_live_values(rows):
    return sorted({0, 1, 4, 5, rows, rows + 3})


# ------------------------------------------------------------------------------------------------ inputs
def _randn(key, *shape):
    return torch.from_numpy(synth.randn(key, shape))


def onehot_k(rows, k, shift=0):
    """k(r) of the one-hot makers: row r holds its one at column (shift + r) mod K."""
    return (torch.arange(rows) + shift) % k


def onehot_shifts(rows, k):
    """The shifts under which `rows` one-hot rows visit every k of every chunk."""
    return tuple(range(0, k, rows))


def onehot_rows(rows, k, shift=0):
    x = torch.zeros(rows, k)
    x[torch.arange(rows), onehot_k(rows, k, shift)] = 1.0
    return x


def gemm_inputs(kind, m, n, k, key="gemm"):
    """(x [m, k], w [n, k], bias [n], bias2 [n]) float32.
    randn: unit x, W / sqrt(K). cancel: x = [a | -a], W = [c | c (1 + 1e-3 e)] with a, c, e > 0: every float64 sum is
    ~5e-4 of its magnitude, reached only after partial sums of the full magnitude (bias scaled to match).
    onehot_x: row r = e_k(r), k(r) = r mod K. onehot_w: the same on the rows of W."""
    tag = f"{key}/{kind}/{m}x{n}x{k}"
    x, w = _randn(tag + "/x", m, k), _randn(tag + "/w", n, k) / math.sqrt(k)
    b, b2 = _randn(tag + "/b", n), _randn(tag + "/b2", n)
    if kind == "cancel":
        h = k // 2
        a, c = x[:, :h].abs() + 0.05, w[:, :h].abs() + 0.05 / math.sqrt(k)
        e = 0.5 + torch.from_numpy(synth._rng(tag + "/e").random_sample((n, h)).astype(np.float32))
        x = torch.cat([a, -a], 1)
        w = torch.cat([c, c * (1 + 1e-3 * e)], 1)
        b, b2 = b * 1e-3, b2 * 1e-3
    elif kind == "onehot_x":
        x = onehot_rows(m, k)
    elif kind == "onehot_w":
        w = onehot_rows(n, k)
    elif kind != "randn":
        raise KeyError(kind)
    return x.contiguous(), w.contiguous(), b, b2


BIG = 2.0 ** 20


def big_row(x, row):
    """x with `row` scaled by 2^20: outside the split window, so its tile takes the second pass; the neighbours stay inside."""
    x = x.clone()
    x[row] *= BIG
    return x


def row_outside_window(x):
    m = x.double().abs().amax(-1)
    return (m >= 2.0 ** 15) | ((m > 0) & (m < 2.0 ** -10))


def ln_inputs(kind, rows, d, key="ln"):
    """(x [rows, d], gamma, beta). offset: mean 30, deviation 1e-2. const: one value per row, each with few enough bits
    that every float32 partial sum of it is exact (variance exactly 0, so the row comes out as beta through eps).
    tiny: deviation 1e-4 about 0 (variance 1e-8: eps dominates)."""
    tag = f"{key}/{kind}/{rows}x{d}"
    x = _randn(tag + "/x", rows, d)
    if kind == "offset":
        x = 30.0 + 1e-2 * x
    elif kind == "const":
        values = torch.tensor([0.0, 30.0, -7.25, 0.5, 1024.0, -3.0, 2.0 ** -12, 100.0])
        x = values[torch.arange(rows) % len(values)][:, None].repeat(1, d)
    elif kind == "tiny":
        x = 1e-4 * x
    elif kind != "randn":
        raise KeyError(kind)
    gamma = 1.0 + 0.5 * _randn(tag + "/g", d)
    beta = _randn(tag + "/be", d)
    return x.contiguous(), gamma, beta


# ------------------------------------------------------------------------------------------------ buffers
def place_x(x, segs, live=None, device="cpu"):
    """The column segments of x [M, K], each a column slice of its own wider NaN-filled buffer: row stride kseg + 8 + 4 s
    floats (a multiple of 4, > kseg, different per segment), base offset 4 (s + 1) floats (16-byte aligned, non-zero).
    Rows at and past `live` hold NaN."""
    x = x.clone()
    if live is not None:
        x[max(0, int(live)):] = float("nan")
    out, k0 = [], 0
    for s, k in enumerate(segs):
        buf = torch.full((x.shape[0] + 1, k + 8 + 4 * s), float("nan"))
        off = 4 * (s + 1)
        buf[:x.shape[0], off:off + k] = x[:, k0:k0 + k]
        out.append(buf.to(device)[:x.shape[0], off:off + k])
        k0 += k
    return out


def place_w(w, contiguous, device="cpu"):
    """W [N, K]: contiguous for the split route (dense.gemm asks for it); otherwise a slice with ldw = K + 4 and NaN behind
    each row and past the last."""
    if contiguous:
        return w.contiguous().to(device)
    buf = torch.full((w.shape[0] + 1, w.shape[1] + 4), float("nan"))
    buf[:w.shape[0], :w.shape[1]] = w
    return buf.to(device)[:w.shape[0], :w.shape[1]]


Out = collections.namedtuple("Out", "buf view col0")


def place_y(m, n, device="cpu", into=None, col0=None):
    """A sentinel-filled buffer of M + 2 rows with 4 columns before and >= 4 after the view [M, N] (row stride a multiple
    of 4 floats, which dense.gemm asks of an output view). `into`: another job's buffer; the view starts at col0 there."""
    if into is None:
        ld = 4 + -(-n // 4) * 4 + 4
        buf = torch.full((m + 2, ld), SENTINEL, device=device)
        col0 = 4
    else:
        buf = into
    return Out(buf, buf[:m, col0:col0 + n], col0)


def outside_intact(buf, regions):
    """True when everything of the sentinel buffer outside `regions` [(rows, col0, n)] still holds the sentinel."""
    mask = torch.ones(buf.shape, dtype=torch.bool)
    for rows, col0, n in regions:
        mask[:rows, col0:col0 + n] = False
    return bool((buf.cpu()[mask] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ judging
def worst_ratio(got, want, mag):
    """max |got - want| / magnitude over the elements with a magnitude; elements without one must be exact."""
    err = (got.double() - want).abs()
    zero = mag == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / mag[~zero]).max())
