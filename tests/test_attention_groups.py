"""Camera-grouped attention (csrc/attention.hip, GROUPED = true) at the group sizes a frame runs, against float64.

The three grouped kernels -- attention_f32_kernel<true> (split=0), attention_f16s_kernel<true> (split=1) and
attention_halfs_kernel<true, 4> (split=2, what a frame runs) -- give each of a workgroup's four waves every fourth 32-key
tile of the key range of its 32 queries. The tables here reach what the 150-slot table of tests/test_gpu_ops.py cannot: a
wave's second and later loop iterations (groups of 129+ and 257+ keys), the next-tile prefetch past a group's end after full
tiles, a query tile that straddles two large groups, all-pad query tiles, empty and one-key groups, and the 48-group flat
slot array of a batch of independent streams.

Reference: _grouped_ref, float64, group by group (no N x N mask). Bounds are the project's own:
  (a) every output finite, rows with query_cam = -1 exactly 0.0;
  (b) max |got - want| <= 2e-5 * max(1, max |want|)                       (test_attention_f32_vs_float64);
  (c) per element |got - want| <= 2e-5 * (P @ |v|), not on the sharp inputs  (test_split_range._check, first line);
  (d) split 1, 2: max error <= 4 x the exact kernel's on the same operands + 1e-7 * max (P @ |v|)   (_check, second line);
  (e) a group's output rows do not change by one bit when every other row of q, k, v is replaced (torch.equal);
  (f) one group over all slots equals the ungrouped launch of the same split within (b).
(c) is not asked of the sharp inputs (|q| |k| / 8 up to ~280, softmax almost one-hot): plain fp32 torch misses it there by
1.1-1.6 x. The CPU test test_fp32_formula_stays_under_half_of_each_bound holds every (table, input) pair to half of each bound
that is applied to it. Measured figures of one MI355X run: profiles/attention_groups_vs_float64.md.

Inputs, E = 512, 8 heads, seeded per (table, input). The ramp strength RAMP is 0.25: with the 0.5 first proposed, plain fp32
on the sharp ramps came to 0.51-0.87 of (b) on r50_frame0, ragged48 and one_group, over the half that the CPU test allows;
with 0.25 the largest is 0.38. The input was changed, not the bound.
  randn                standard normal q, k, v;
  ramp_up / ramp_down  q + RAMP u and k + RAMP r u with u one random direction, r rising (falling) linearly 0..1 over the slots;
  sharp_*              the same three, q, k and v times 4;
  grow / decay         k rows times 0.1^j (decay) or 0.1^(jmax - j) (grow), j = (position in the group) // 128: a wave's
                       tiles are 128 keys apart, so under decay every query's maximum is set in its wave's first tile and never
                       moves (logits of the next tile are ~10x smaller: the halfs kernel's no-rescale branch in every later
                       iteration), and under grow it moves in every iteration. Magnitudes only shrink, so (c) applies."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.test_gpu_ops import _pack_split_halfs

gpu = pytest.mark.gpu
HEADS, E = 8, 512


# ---------------------------------------------------------------------------------------------------- tables
def _r50_bounds():
    g = load_golden("head_r50.npz")["f0.trace.L00.allocation.query_groups#0"]   # [cams, 2]: (start, end) per camera
    assert bool((g[1:, 0] == g[:-1, 1]).all())
    return [int(g[0, 0])] + [int(e) for e in g[:, 1]]


def _ragged48_bounds():
    """8 independent streams x 6 cameras in one flat slot array (stream-major, as simpb_alloc_ragged lays it out): stream s
    holds the six r50_frame0 group sizes rotated by s; the capacity slots follow the last group."""
    sizes = np.diff(np.asarray(_r50_bounds()))
    return [0] + [int(c) for c in np.cumsum(np.concatenate([np.roll(sizes, s) for s in range(8)]))]


_TABLES = {}


def _table(name):
    """(bounds, N): group c is slots [bounds[c], bounds[c + 1]); slots past bounds[-1] are capacity."""
    if name not in _TABLES:
        _TABLES[name] = {
            "r50_frame0": lambda: (_r50_bounds(), 1536),
            "edges": lambda: ([0, 1, 32, 64, 97, 97, 225, 354, 514, 771, 771, 800], 832),
            "ragged48": lambda: (_ragged48_bounds(), 8 * 1280),
            "one_group": lambda: ([0, 900], 900),
            "no_group": lambda: ([0, 0, 0, 0, 0, 0, 0], 96),
        }[name]()
    return _TABLES[name]


TABLES = ["r50_frame0", "edges", "ragged48", "one_group", "no_group"]
INPUTS = ["randn", "ramp_up", "ramp_down", "sharp_randn", "sharp_ramp_up", "sharp_ramp_down", "grow", "decay"]
RAMP = 0.25


def _query_cam(bounds, n):
    cam = torch.full((n,), -1, dtype=torch.int32)
    for c in range(len(bounds) - 1):
        cam[bounds[c]:bounds[c + 1]] = c
    return cam


def _inputs(table, kind, bs=1):
    bounds, n = _table(table)
    g = torch.Generator().manual_seed(100 * TABLES.index(table) + INPUTS.index(kind) + 1)
    q, k, v = (torch.randn(bs, n, E, generator=g) for _ in range(3))
    base = kind[6:] if kind.startswith("sharp_") else kind
    if base in ("ramp_up", "ramp_down"):
        u = torch.randn(E, generator=g)
        r = torch.linspace(0, 1, n) if base == "ramp_up" else torch.linspace(1, 0, n)
        q = q + RAMP * u
        k = k + RAMP * r[None, :, None] * u
    elif base in ("grow", "decay"):
        f = torch.ones(n)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            if hi > lo:
                j = torch.arange(hi - lo) // 128
                f[lo:hi] = 0.1 ** ((j if base == "decay" else int(j[-1]) - j).float())
        k = k * f[None, :, None]
    if kind.startswith("sharp_"):
        q, k, v = q * 4, k * 4, v * 4
    return q, k, v


# ---------------------------------------------------------------------------------------------------- reference
def _grouped_ref(q, k, v, bounds, heads, dtype=torch.float64):
    """(want, mag): per group [lo, hi) plain softmax(q[lo:hi] k[lo:hi]^T / sqrt(hd)) v[lo:hi] per head, zeros outside every
    group; mag = P @ |v|. Evaluated in `dtype` (float64: the reference; float32: what plain fp32 arithmetic gives)."""
    bs, n, e = q.shape
    hd = e // heads
    want = torch.zeros(bs, n, e, dtype=dtype)
    mag = torch.zeros(bs, n, e, dtype=dtype)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        if hi <= lo:
            continue
        qg, kg, vg = (t[:, lo:hi].to(dtype).reshape(bs, hi - lo, heads, hd).transpose(1, 2) for t in (q, k, v))
        p = torch.softmax(qg @ kg.transpose(-1, -2) / math.sqrt(hd), -1)
        want[:, lo:hi] = (p @ vg).transpose(1, 2).reshape(bs, hi - lo, e)
        mag[:, lo:hi] = (p @ vg.abs()).transpose(1, 2).reshape(bs, hi - lo, e)
    return want, mag


_REF = {}


def _case(table, kind):
    """Operands and their float64 reference, computed once per (table, input)."""
    if (table, kind) not in _REF:
        _REF.clear()   # one entry: a pair's splits run back to back, and ragged48 is ~250 MB per pair
        q, k, v = _inputs(table, kind)
        _REF[table, kind] = (q, k, v) + _grouped_ref(q, k, v, _table(table)[0], HEADS)
    return _REF[table, kind]


def _ratios(got, want, mag):
    """Error as a fraction of bound (b) and of bound (c)."""
    err = (got.double() - want).abs()
    rb = float(err.max()) / (2e-5 * max(1.0, float(want.abs().max()))) if err.numel() else 0.0
    rc = float((err / (2e-5 * mag).clamp_min(1e-300)).max()) if err.numel() else 0.0
    return rb, rc


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", TABLES)
def test_table_builder(name):
    bounds, n = _table(name)
    cam = _query_cam(bounds, n)
    assert bounds[0] == 0 and all(a <= b for a, b in zip(bounds[:-1], bounds[1:])) and bounds[-1] <= n
    assert cam.dtype == torch.int32 and cam.shape == (n,)
    assert bool((cam[bounds[-1]:] == -1).all()) and bool((cam[:bounds[-1]] >= 0).all())
    for c in range(len(bounds) - 1):   # query_cam consistent with group_start: group c is exactly its contiguous range
        assert torch.nonzero(cam == c).flatten().tolist() == list(range(bounds[c], bounds[c + 1]))
    sizes = [b - a for a, b in zip(bounds[:-1], bounds[1:])]
    if name == "r50_frame0":
        assert len(sizes) == 6 and min(sizes) >= 129 and n - bounds[-1] == 406
        assert sum(1 for t in range(0, n, 32) if t >= bounds[-1]) == 12          # all-pad query tiles
        assert any(b % 32 for b in bounds[1:-1])                                  # straddling query tiles
    if name == "edges":
        assert sizes == [1, 31, 32, 33, 0, 128, 129, 160, 257, 0, 29]
        assert sum(1 for t in range(0, n, 32) if t >= bounds[-1]) == 1
        assert bounds[6] // 32 == (bounds[6] - 1) // 32 and bounds[7] // 32 == (bounds[7] - 1) // 32   # 225 and 354 inside a tile
    if name == "ragged48":
        assert len(sizes) == 48 and n - bounds[-1] == 1200 and max(bounds) > 9000
        r50 = sorted(b - a for a, b in zip(_r50_bounds()[:-1], _r50_bounds()[1:]))
        assert all(sorted(sizes[6 * s:6 * s + 6]) == r50 for s in range(8)) and sizes[6:12] != sizes[:6]
    if name == "no_group":
        assert bool((cam == -1).all())


def test_grouped_ref_equals_dense_mask_formulation():
    """On the 150-slot table: the reference's own formulation (group_attn.py:104-131: dense scores + additive -inf block mask +
    nan_to_num) as tests/test_split_range.py writes it (it takes q with the 1/8 folded in: a power of two, exact)."""
    from tests.test_split_range import _BOUNDS, _att_ref
    g = torch.Generator().manual_seed(31)
    q, k, v = (torch.randn(1, 150, E, generator=g) for _ in range(3))
    want, mag = _grouped_ref(q, k, v, _BOUNDS, HEADS)
    dense_want, dense_mag = _att_ref(q / 8, k, v, True)
    assert want.dtype == torch.float64 and mag.dtype == torch.float64
    assert float((want - dense_want).abs().max()) <= 1e-12 and float((mag - dense_mag).abs().max()) <= 1e-12
    assert bool((want[:, _BOUNDS[-1]:] == 0).all()) and bool((mag[:, _BOUNDS[-1]:] == 0).all()) and float(want.abs().max()) > 0.1


def test_one_group_ref_equals_ungrouped_float64():
    q, k, v, want, _ = _case("one_group", "randn")
    qd, kd, vd = (t.double().reshape(1, 900, HEADS, 64).transpose(1, 2) for t in (q, k, v))
    plain = (torch.softmax(qd @ kd.transpose(-1, -2) / 8.0, -1) @ vd).transpose(1, 2).reshape(1, 900, E)
    assert float((want - plain).abs().max()) <= 1e-12


@pytest.mark.parametrize("kind", ["decay", "grow"])
def test_decay_and_grow_move_the_running_maximum_as_described(kind):
    """In float64, per wave of a workgroup whose 32 queries lie inside one group: under decay no query's running maximum
    moves after the wave's first tile, under grow every query's moves in every later tile."""
    q, k, _, _, _ = _case("r50_frame0", kind)
    bounds, _ = _table("r50_frame0")
    lo, hi = bounds[2], bounds[3]
    t0 = (lo + 31) // 32 * 32   # first query tile inside the group
    s = (q[0, t0:t0 + 32].double().reshape(32, HEADS, 64).transpose(0, 1) @
         k[0, lo:hi].double().reshape(hi - lo, HEADS, 64).permute(1, 2, 0)) / 8.0   # [heads, 32, keys]
    for wave in range(4):
        tiles = [s[..., a:a + 32].amax(-1) for a in range(32 * wave, hi - lo, 128)]
        assert len(tiles) >= 2 or 32 * wave + 128 >= hi - lo
        run = tiles[0]
        for t in tiles[1:]:
            assert bool((t < run).all()) if kind == "decay" else bool((t > run).all())
            run = torch.maximum(run, t)


def _strided_inputs():
    g = torch.Generator().manual_seed(77)
    return torch.randn(2, _table("edges")[1], 3 * E, generator=g)


def _chain_inputs():
    """x, the q|k|v weight with the softmax scale folded into its q rows (plugin/layers.py:173-189), bias, and q, k, v in
    float64 from x: the live rows only, capacity rows zeros (what the GEMM writes past *m_live)."""
    bounds, n = _table("r50_frame0")
    g = torch.Generator().manual_seed(78)
    x = torch.randn(1, n, E, generator=g)
    w = torch.randn(3 * E, E, generator=g) / math.sqrt(E)
    bias = torch.randn(3 * E, generator=g) * 0.1
    rs = torch.cat([torch.full((E,), 0.125), torch.ones(2 * E)])
    w, bias = w * rs[:, None], bias * rs
    qkv = torch.zeros(1, n, 3 * E, dtype=torch.float64)
    qkv[0, :bounds[-1]] = x[0, :bounds[-1]].double() @ w.double().t() + bias.double()
    return x, w, bias, (qkv[..., :E] * 8.0, qkv[..., E:2 * E], qkv[..., 2 * E:])   # the unscaled q for the reference


def _all_cases():
    for table in TABLES:
        for kind in INPUTS:
            yield (table, kind), _table(table)[0], _case(table, kind), not kind.startswith("sharp_")
    buf = _strided_inputs()
    q, k, v = buf[..., :E], buf[..., E:2 * E], buf[..., 2 * E:]
    bounds = _table("edges")[0]
    yield ("edges", "bs2_strided"), bounds, (q, k, v) + _grouped_ref(q, k, v, bounds, HEADS), True
    q, k, v = _chain_inputs()[3]
    bounds = _table("r50_frame0")[0]
    yield ("r50_frame0", "chain"), bounds, (q.float(), k.float(), v.float()) + _grouped_ref(q, k, v, bounds, HEADS), True


def test_fp32_formula_stays_under_half_of_each_bound():
    """The same per-group formula in plain fp32 torch stays under HALF of every bound the GPU tests apply to that pair:
    (b) everywhere, (c) on the non-sharp inputs. So a correct fp32-grade kernel can meet them."""
    over = []
    for what, bounds, (q, k, v, want, mag), with_c in _all_cases():
        got, _ = _grouped_ref(q, k, v, bounds, HEADS, dtype=torch.float32)
        rb, rc = _ratios(got, want, mag)
        print("fp32 %s %s: (b) %.3f (c) %.3f%s" % (what + (rb, rc, "" if with_c else " (not applied)")))
        if rb > 0.5 or (with_c and rc > 0.5):
            over.append((what, rb, rc))
    assert not over, over


# ---------------------------------------------------------------------------------------------------- GPU
def _run(q, k, v, split, tables=()):
    """One launch on fp32 operands [bs, N, E]; split=2: packed as the producing GEMM leaves them, 1/8 folded into q."""
    from simpb_amd.plugin.ops import attention_f32
    if split == 2:
        q, k, v = (_pack_split_halfs(t.contiguous()) for t in (q * 0.125, k, v))
    return attention_f32(q.cuda(), k.cuda(), v.cuda(), HEADS, *tables, split=split).cpu()


def _device_tables(bounds, n):
    return _query_cam(bounds, n).cuda(), torch.tensor(bounds, dtype=torch.int32).cuda()


def _check(got, exact, want, mag, cam, with_c, what):
    """(a)-(d); `exact` is the split=0 output on the same operands (None when `got` is that output)."""
    assert bool(torch.isfinite(got).all()), (what, "non-finite output", int((~torch.isfinite(got)).sum()))
    assert bool((got[:, cam < 0] == 0).all()), (what, "capacity rows not exactly zero")
    rb, rc = _ratios(got, want, mag)
    err = float((got.double() - want).abs().max()) if got.numel() else 0.0
    rd = 0.0
    if exact is not None:
        e_exact = float((exact.double() - want).abs().max())
        rd = err / (4 * e_exact + 1e-7 * float(mag.max())) if err else 0.0
    print("RATIO|%s|%s|split%d|b=%.3f|c=%.3f%s|d=%.3f" % (what[0], what[1], what[2], rb, rc, "" if with_c else "(n/a)", rd))
    assert rb <= 1.0, (what, "max error / (2e-5 * max(1, max |want|))", rb)
    if with_c:
        assert rc <= 1.0, (what, "error / (2e-5 * P @ |v|)", rc)
    assert rd <= 1.0, (what, "max error / (4 x exact kernel's + 1e-7 max mag)", rd)


_EXACT = {}


def _exact_of(key, q, k, v, tables):
    if key not in _EXACT:
        _EXACT.clear()
        _EXACT[key] = _run(q, k, v, 0, tables)
    return _EXACT[key]


@gpu
@pytest.mark.parametrize("split", [0, 1, 2])
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("table", TABLES)
def test_grouped_attention_vs_float64(table, kind, split):
    bounds, n = _table(table)
    q, k, v, want, mag = _case(table, kind)
    tables = _device_tables(bounds, n)
    exact = _exact_of((table, kind), q, k, v, tables)
    got = exact if split == 0 else _run(q, k, v, split, tables)
    _check(got, None if split == 0 else exact, want, mag, _query_cam(bounds, n), not kind.startswith("sharp_"),
           (table, kind, split))
    if table == "no_group":
        assert bool((got == 0).all())


@gpu
@pytest.mark.parametrize("split", [0, 1, 2])
@pytest.mark.parametrize("kind", INPUTS)
def test_one_group_equals_the_ungrouped_launch(kind, split):
    """(f): same operands, same split, without tables (for split=2 the eight-wave form): summation order only."""
    bounds, n = _table("one_group")
    q, k, v, want, _ = _case("one_group", kind)
    grouped = _run(q, k, v, split, _device_tables(bounds, n))
    plain = _run(q, k, v, split)
    bound = 2e-5 * max(1.0, float(want.abs().max()))
    for name, a, b in (("grouped - ungrouped", grouped.double(), plain.double()), ("ungrouped - float64", plain.double(), want)):
        r = float((a - b).abs().max()) / bound
        print("RATIO|one_group|%s|split%d|%s|b=%.3f" % (kind, split, name, r))
        assert r <= 1.0, (kind, split, name, r)


@gpu
@pytest.mark.parametrize("split", [0, 1, 2])
def test_grouped_attention_bs2_strided_views_vs_float64(split):
    """bs = 2 on `edges`, q / k / v as column ranges of one [bs, N, 1536] buffer, as the fused projection hands them over."""
    from simpb_amd.plugin.ops import attention_f32
    bounds, n = _table("edges")
    buf = _strided_inputs()
    q, k, v = buf[..., :E], buf[..., E:2 * E], buf[..., 2 * E:]
    want, mag = _grouped_ref(q, k, v, bounds, HEADS)
    tables = _device_tables(bounds, n)
    dev = buf.cuda()
    exact = attention_f32(dev[..., :E], dev[..., E:2 * E], dev[..., 2 * E:], HEADS, *tables, split=0).cpu()
    if split == 2:
        dev = torch.cat([_pack_split_halfs(buf[..., :E] * 0.125), _pack_split_halfs(buf[..., E:].contiguous())], -1).cuda()
    got = exact if split == 0 else attention_f32(dev[..., :E], dev[..., E:2 * E], dev[..., 2 * E:], HEADS, *tables, split=split).cpu()
    assert dev[..., :E].stride() == (n * 3 * E, 3 * E, 1)
    _check(got, None if split == 0 else exact, want, mag, _query_cam(bounds, n), True, ("edges", "bs2_strided", split))


@gpu
def test_shipped_chain_at_shipped_size_vs_float64():
    """The q|k|v GEMM with split_halfs output and *m_live = 1130 into attention_halfs_kernel<true, 4> over 1536 slots,
    against float64 computed from x; the capacity rows are the zeros the GEMM writes."""
    from simpb_amd.plugin import dense
    from simpb_amd.plugin.ops import attention_f32
    bounds, n = _table("r50_frame0")
    x, w, bias, (q, k, v) = _chain_inputs()
    want, mag = _grouped_ref(q, k, v, bounds, HEADS)
    tables = _device_tables(bounds, n)
    live = torch.tensor([bounds[-1]], dtype=torch.int32, device="cuda")
    packed = dense.linear([x.cuda()], w.cuda(), bias.cuda(), m_live=live, split_halfs=True)
    assert bool((packed[0, bounds[-1]:].view(torch.int32) == 0).all())
    got = attention_f32(packed[..., :E], packed[..., E:2 * E], packed[..., 2 * E:], HEADS, *tables, split=2).cpu()
    exact = _run(q.float(), k.float(), v.float(), 0, tables)
    _check(got, exact, want, mag, _query_cam(bounds, n), True, ("r50_frame0", "chain", 2))


@gpu
@pytest.mark.parametrize("split", [0, 1, 2])
@pytest.mark.parametrize("table,group", [("edges", 6), ("r50_frame0", 2)])
def test_group_output_is_bitwise_independent_of_other_rows(table, group, split):
    """(e): the chosen group shares its first and last query tile with its neighbours. Masked scores become -inf by a select
    before they are used (exp = 0 exactly), 0 x finite = 0 in the second product, the table and so the tiling is unchanged,
    and a rescale by alpha == 1 is the identity: replacing every other row of q, k, v (other groups and capacity slots) by
    fresh random values times 64 -- finite in half precision, also times 1/8 -- must not change one bit of the group's rows."""
    bounds, n = _table(table)
    lo, hi = bounds[group], bounds[group + 1]
    assert lo % 32 and hi % 32 and bounds[group] - bounds[group - 1] >= 128 and bounds[group + 2] - hi >= 128
    q, k, v, _, _ = _case(table, "randn")
    g = torch.Generator().manual_seed(91)
    poisoned = []
    for t in (q, k, v):
        p = torch.randn(t.shape, generator=g) * 64
        p[:, lo:hi] = t[:, lo:hi]
        poisoned.append(p)
    assert all(bool(torch.isfinite(p.half()).all()) for p in poisoned)
    tables = _device_tables(bounds, n)
    clean = _run(q, k, v, split, tables)
    dirty = _run(*poisoned, split, tables)
    assert bool(torch.isfinite(dirty).all())
    assert not torch.equal(clean[:, :lo], dirty[:, :lo])   # the poison did reach the kernel
    assert torch.equal(clean[:, lo:hi], dirty[:, lo:hi]), (
        table, split, "rows of the group that changed", int((clean[:, lo:hi] != dirty[:, lo:hi]).any(-1).sum()))
