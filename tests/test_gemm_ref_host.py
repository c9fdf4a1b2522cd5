"""tests/gemm_ref.py without a GPU: the float64 models against torch's float64 operators, the route twin against the case
tables of tests/test_gemm_float64.py (every case reaches the kernel it is named for, every listed edge is present), a plain
float32 evaluation under HALF of every bound those cases are held to, and the inputs being what they claim."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as G

ROUTE_NAMES = list(G.ROUTES)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ models agree with torch
@pytest.mark.parametrize("kind", ["randn", "cancel", "onehot_x", "onehot_w"])
def test_gemm_ref_matches_torch_float64(kind):
    x, w, b, b2 = G.gemm_inputs(kind, 70, 65, 320)
    flags = (torch.arange(70) % 2).int()
    y, mag = G.gemm_ref([x[:, :64], x[:, 64:]], w, b, relu=True, live=41, row_flag=flags, bias2=b2)
    want = F.relu(F.linear(x.double(), w.double(), b.double()) + flags.double()[:, None] * b2.double())
    assert _rel(y[:41], want[:41]) <= 1e-12 and bool((y[41:] == 0).all()) and bool((mag[41:] == 0).all())
    assert bool((mag[:41] >= (y[:41].abs() - 1e-12)).all())
    y0, _ = G.gemm_ref([x], w)
    assert _rel(y0, F.linear(x.double(), w.double())) <= 1e-12
    full = G.products(x, w)   # a slice of a larger product serves a smaller case
    ys, ms = G.gemm_ref([x[:33]], w[:40], b[:40], relu=True, live=20, product=(full[0][:33, :40], full[1][:33, :40]))
    yd, md = G.gemm_ref([x[:33]], w[:40], b[:40], relu=True, live=20)
    assert _rel(ys, yd) <= 1e-12 and _rel(ms, md) <= 1e-12 and bool((ys[20:] == 0).all())


@pytest.mark.parametrize("kind", G.LN_KINDS)
def test_layernorm_ref_matches_torch_float64(kind):
    x, g, b = G.ln_inputs(kind, 5, 512)
    y, _ = G.layernorm_ref([x[:, :64], x[:, 64:]], g, b, live=4)
    want = F.layer_norm(x.double(), (512,), g.double(), b.double(), 1e-5)
    assert float((y[:4] - want[:4]).abs().max()) <= 1e-12 * float(want.abs().max()) + 1e-9 * (kind == "offset")
    assert bool((y[4:] == 0).all())


def test_rowdot_ref_matches_torch_float64():
    x, w, _, _ = G.gemm_inputs("randn", 301, 1, 260, key="rowdot")
    for bias in (0.3, 100.0, -100.0):
        b = torch.tensor([bias])
        y = G.rowdot_sigmoid_ref(x, w, b, live=300)
        want = torch.sigmoid(x.double() @ w.double().t() + float(b))
        assert _rel(y[:300], want[:300]) <= 1e-12 and float(y[300]) == 0.0 and bool(torch.isfinite(y).all())


def test_halfs_round_trip():
    y = torch.cat([G._randn("halfs", 4096), torch.tensor([0.0, 1.0, -2.5, 1e-3, 60000.0])])
    back = G.halfs_value(G.halfs_word(y))
    assert bool((back[y == 0] == 0).all())
    assert bool(((back - y.double()).abs() <= G.PLACE_SPLIT * y.double().abs().clamp_min(G.HALF_MIN_NORMAL)).all())


# ------------------------------------------------------------------------------------------------ routes are reached
def _all_gemm_cases(route):
    return G.sweep_cases(route) + G.chunk_cases(route)


@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_every_named_case_reaches_its_kernel(route):
    split = G.exact_split(route)
    for m, n, segs, _, _ in _all_gemm_cases(route):
        assert G.route_of([G.job_dims(m, n, segs)], split).name == route, (m, n, segs)
    m, n = G.SEGMENT_SHAPE[route]
    comps = G.segment_cases(route)
    assert comps
    for segs in comps:
        assert G.route_of([G.job_dims(m, n, segs)], split).name == route, segs
    rm, rn = G.SWEEP[route]["ragged"]
    assert G.route_of([G.job_dims(rm, rn, G.SWEEP[route]["segs"])], split).name == route
    assert -(-rm // G.ROUTES[route].tile_m) >= 3 and rm % G.ROUTES[route].tile_m and rn % G.ROUTES[route].tile_n
    if G.ROUTES[route].split:   # a weight outside the window, a strided weight or the switch: the exact kernel
        d = G.job_dims(rm, rn, G.SWEEP[route]["segs"])
        for off in (dict(w_in_window=False), dict(w_contiguous=False)):
            assert not G.route_of([dict(d, **off)], True).split
        assert not G.route_of([d], False).split


def test_each_group_has_each_route():
    grouped = {G.GROUPED[c][0] for c in G.GROUPED}
    assert grouped == set(ROUTE_NAMES)
    for case, (route, jobs) in G.GROUPED.items():
        assert G.route_of(G.grouped_dims(case), G.exact_split(route)).name == route, case
        assert 1 <= len(jobs) <= 4
    assert {len(j) for _, j in G.GROUPED.values()} == {1, 2, 3, 4}
    wide = G.GROUPED["wide_four_jobs"][1]
    assert len(wide) == 4   # only together past the 400 tiles
    for drop in range(4):
        rest = [G.job_dims(*j[:3]) for i, j in enumerate(wide) if i != drop]
        assert G.route_of(rest, True).name != "f16_wide", drop


def test_route_thresholds():
    """The two tile thresholds and the K rule, one below and at each."""
    assert G.route_of([G.job_dims(32 * 10, 64 * 20 - 64, (64,))], False).name == "f32_d4k64"      # 190 tiles
    assert G.route_of([G.job_dims(32 * 10, 64 * 20, (64,))], False).name == "f32_n64"             # 200
    assert G.route_of([G.job_dims(64 * 20, 128 * 20 - 128, (128,))], True).name == "f16_n64"      # 380
    assert G.route_of([G.job_dims(64 * 20, 128 * 20, (128,))], True).name == "f16_wide"           # 400
    assert G.route_of([G.job_dims(33, 33, (384,))], False).name == "f32_d4k64"
    assert G.route_of([G.job_dims(33, 33, (512,))], False).name == "f32_d2k128"
    assert G.route_of([G.job_dims(33, 33, (64, 448))], False).name == "f32_d4k64"
    assert G.route_of([G.job_dims(33, 33, (512,)), G.job_dims(33, 33, (256,))], False).name == "f32_d4k64"
    assert G.route_of([G.job_dims(33, 33, (128,)), G.job_dims(33, 33, (64, 64))], True).name == "f32_d4k64"


# ------------------------------------------------------------------------------------------------ edges are present
@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_tables_hold_the_listed_edges(route):
    r, t = G.ROUTES[route], G.SWEEP[route]
    for values, tile in ((t["ms"], r.tile_m), (t["ns"], r.tile_n)):
        mods = {v % tile for v in values}
        assert {tile - 1, 0, 1} <= mods, (values, tile)
        if route in ("f32_d4k64", "f32_d2k128", "f16_d2k128"):
            assert {1, 31, 32, 33, 63, 65} <= set(values)
        elif tile > 32:
            assert any(v % tile == 33 for v in values)   # a partial tile of 32 + 1
    assert set(G.REQUIRED_CHUNKS[route]) <= set(t["chunks"])
    for c in t["chunks"]:
        assert sum(G.chunk_segs(route, c)) == c * r.chunk
    if route == "f16_wide":
        assert all(c % 2 == 0 for c in t["chunks"])   # the wide kernel's loop has no tail: the split route keeps K % 128 == 0
    assert {0, 1, r.tile_m - 1, r.tile_m, r.tile_m + 1, t["ragged"][0] - 1, t["ragged"][0], t["ragged"][0] + 5} == set(G.live_values(route))
    # segment boundaries: every chunk index that can carry one does, at K = 256 and K = 512
    comps = G.segment_cases(route)
    for k in (256, 512):
        cuts = {c // r.chunk for s in comps if sum(s) == k for c in itertools.accumulate(s[:-1]) if c % r.chunk == 0}
        want = {c // r.chunk for s in G.compositions(k, 64 if route in ("f32_d4k64", "f32_n64") else 128)
                if G.route_of([G.job_dims(*G.SEGMENT_SHAPE[route], s)], r.split).name == route
                for c in itertools.accumulate(s[:-1]) if c % r.chunk == 0}
        assert cuts == want and (want or k == 256), (k, cuts, want)
    assert {len(s) for s in comps} >= {1, 2, 3, 4}


def test_grouped_totals_hold_the_listed_remainders():
    totals = {c: G.total_tiles(G.grouped_dims(c), G.exact_split(G.GROUPED[c][0])) for c in G.GROUPED}
    assert set(G.REQUIRED_TOTALS) <= set(totals.values()), totals
    assert {0, 1, 7} <= {t % 8 for t in totals.values()}, totals
    jobs = [j for _, js in G.GROUPED.values() for j in js]
    assert any(j[0] < 32 for j in jobs)
    assert any(js[i][5] == "capacity" and 0 < i < len(js) - 1 for _, js in G.GROUPED.values() for i in range(len(js)))
    assert any(j[5] == "adjacent" for j in jobs) and any(j[5] == "flags" for j in jobs)
    case = "four_jobs"   # a job's first tile inside an XCD's range, not only at its start
    r = G.ROUTES[G.GROUPED[case][0]]
    starts = list(itertools.accumulate(G.tiles([d], r.tile_m, r.tile_n) for d in G.grouped_dims(case)))
    per_xcd = -(-starts[-1] // 8)
    assert any(s % per_xcd for s in starts[:-1]), (starts, per_xcd)


def test_row_kernel_tables():
    assert set(G.LN_WIDTHS) == {(64, 0), (256, 0), (512, 0), (256, 256), (64, 448), (320, 64)}
    assert G.LN_ROWS == (1, 3, 4, 5, 301) == G.ROWDOT_ROWS and G.ROWDOT_K == (4, 252, 256, 260, 512)
    assert G.rows_live_values(301) == [0, 1, 4, 5, 301, 304]
    assert G.LINEAR_M == (1, 63, 64, 65, 129) and G.LINEAR_N == (1, 255, 256, 257, 513) and G.LINEAR_K == (32, 64, 96)


# ------------------------------------------------------------------------------------------------ plain fp32 under half
def _fp32_ratio(x, w, b, relu):
    want, mag = G.gemm_ref([x], w, b, relu)
    got = x.float() @ w.float().t()
    if b is not None:
        got = got + b.float()
    if relu:
        got = got.clamp_min(0)
    return G.worst_ratio(got, want, mag)


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_plain_fp32_is_under_half_of_the_element_bound(route, kind, record_property):
    """Bound (b) on the operands of the tile sweep (their full extent: every case is a slice of it), of every chunk count
    and of every segment case (the same K = 256 / 512 operands)."""
    t = G.SWEEP[route]
    worst = 0.0
    shapes = [(max(t["ms"]), max(t["ns"]), sum(t["segs"]))]
    shapes += [(*t["ragged"], G.ROUTES[route].chunk * c) for c in t["chunks"]]
    shapes += [(*G.SEGMENT_SHAPE[route], k) for k in (256, 512)]
    for m, n, k in shapes:
        x, w, b, _ = G.gemm_inputs(kind, m, n, k)
        assert G.in_window(w)   # the split routes take these weights; the exact ones run them all the same
        if route == "f16_wide":   # rows are independent: a band of them bounds the float32 evaluation as well
            x = x[:160]
        for bias, relu in ((b, False), (None, True)):
            worst = max(worst, _fp32_ratio(x, w, bias, relu))
    record_property("worst_fp32_ratio", worst)
    print(f"FIG fp32 {route} {kind} worst err/magnitude = {worst:.3e} (bound {G.REL:.0e})")
    assert worst <= G.REL / 2


@pytest.mark.parametrize("case", list(G.GROUPED))
def test_plain_fp32_is_under_half_on_the_grouped_jobs(case):
    """The operands of every grouped job (as tests/test_gemm_float64.py makes them), with their flags and second bias;
    on a split route every weight lies inside the split window, or the launch would leave the route."""
    for j, (m, n, segs, bias, relu, extra) in enumerate(G.GROUPED[case][1]):
        x, w, b, b2 = G.gemm_inputs("randn", m, n, sum(segs), key=f"grouped/{case}/{j}")
        assert G.in_window(w) or not G.ROUTES[G.GROUPED[case][0]].split
        flags = ((torch.arange(m) % 3) == 0).int() if extra == "flags" else None
        want, mag = G.gemm_ref([x], w, b if bias else None, relu, None, flags, b2 if flags is not None else None)
        got = x @ w.t()
        if bias:
            got = got + b
        if flags is not None:
            got = got + flags.float()[:, None] * b2
        assert G.worst_ratio(got.clamp_min(0) if relu else got, want, mag) <= G.REL / 2, (case, j)


@pytest.mark.parametrize("route", list(G.EXACT_ROUTES))
def test_plain_fp32_places_onehot_exactly(route):
    """Bound (d): float32 arithmetic on a one-hot row is one rounding, the sum of the bias."""
    m, n = G.SWEEP[route]["ragged"]
    k = sum(G.SWEEP[route]["segs"])
    x, w, b, _ = G.gemm_inputs("onehot_x", m, n, k)
    got = x @ w.t() + b
    assert torch.equal(got, w[:, G.onehot_k(m, k)].t() + b)
    want, _ = G.gemm_ref([x], w, b)
    assert float((got.double() - want).abs().max()) <= 2.0 ** -24 * float(want.abs().max())


@pytest.mark.parametrize("kind", G.LN_KINDS)
def test_plain_fp32_layernorm_under_half(kind):
    """randn: absolute 2e-5. The other kinds are held to 4 e32 + 1e-7 max magnitude on the GPU, e32 being this very
    evaluation; here: e32 is finite, and const rows come out as beta exactly (their variance is exactly 0 in float32)."""
    for (k0, k1), rows in itertools.product(G.LN_WIDTHS, (5, 301)):
        x, g, b = G.ln_inputs(kind, rows, k0 + k1)
        want, mag = G.layernorm_ref([x], g, b)
        got = G.layernorm_f32([x], g, b)
        err = float((got.double() - want).abs().max())
        assert math.isfinite(err)
        if kind == "randn":
            assert err <= G.LN_ABS / 2, (k0, k1, rows, err)
        if kind == "const":
            assert torch.equal(got, b.expand_as(got)) and err == 0.0
        if kind == "tiny":
            assert err <= G.LN_ABS / 2


def test_plain_fp32_rowdot_under_half():
    for k, rows in itertools.product(G.ROWDOT_K, (5, 301)):
        x, w, _, _ = G.gemm_inputs("randn", rows, 1, k, key="rowdot")
        for bias in (0.3, 100.0, -100.0):
            want = G.rowdot_sigmoid_ref(x, w, torch.tensor([bias]))
            got = torch.sigmoid(x @ w.t() + bias)
            assert bool(torch.isfinite(got).all())
            assert float((got.double() - want).abs().max()) <= G.ROWDOT_ABS / 2
            if bias == 100.0:
                assert bool((got == 1).all())
            if bias == -100.0:
                assert bool((got < 1e-30).all())


# ------------------------------------------------------------------------------------------------ inputs are what they claim
def test_cancel_rows_cancel():
    x, w, b, _ = G.gemm_inputs("cancel", 70, 65, 512)
    want, mag = G.gemm_ref([x], w)
    ratio = want.abs() / mag
    assert float(ratio.max()) <= 1e-3 and float(ratio.min()) >= 1e-4
    half = x[:, :256].double() @ w[:, :256].double().t()
    assert float((half.abs() / mag).min()) >= 0.4   # the partial sum reaches the full magnitude before it cancels


def test_big_row_is_outside_the_window_and_its_neighbours_inside():
    x, _, _, _ = G.gemm_inputs("randn", 70, 65, 256)
    for row in (0, 17, 31, 69):
        out = G.row_outside_window(G.big_row(x, row))
        assert bool(out[row]) and int(out.sum()) == 1


@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_onehot_walks_every_k(route):
    for m, _, segs, _, _ in G.chunk_cases(route) + [(*G.SEGMENT_SHAPE[route], s, 0, 0) for s in G.segment_cases(route)]:
        k = sum(segs)
        seen = set()
        for shift in G.onehot_shifts(m, k):
            x = G.onehot_rows(m, k, shift)
            assert bool((x.sum(1) == 1).all()) and bool(((x == 0) | (x == 1)).all())
            seen |= set(G.onehot_k(m, k, shift).tolist())
        assert seen == set(range(k)), (m, k)


def test_ln_inputs_are_what_they_claim():
    x, _, _ = G.ln_inputs("offset", 301, 512)
    assert abs(float(x.double().mean()) - 30) < 1e-2 and 0.5e-2 < float(x.double().std(1).mean()) < 2e-2
    x, _, _ = G.ln_inputs("const", 301, 512)
    assert bool((x == x[:, :1]).all()) and len(set(x[:, 0].tolist())) >= 8
    assert torch.equal(x.sum(1), x[:, 0] * 512)   # float32 partial sums exact
    x, _, _ = G.ln_inputs("tiny", 301, 512)
    assert float(x.double().var(1, unbiased=False).max()) < 1e-7 < 1e-5


def test_buffers_put_operands_among_nan_and_sentinels():
    x, w, _, _ = G.gemm_inputs("randn", 33, 40, 512)
    segs = (64, 128, 256, 64)
    xs = G.place_x(x, segs, live=20)
    assert [t.shape[1] for t in xs] == list(segs)
    assert len({t.stride(0) for t in xs}) == 4 and len({t.storage_offset() for t in xs}) == 4
    for s, t in enumerate(xs):
        assert t.stride(0) % 4 == 0 and t.stride(0) > segs[s] and t.stride(1) == 1
        assert t.storage_offset() % 4 == 0 and t.storage_offset() > 0
        assert bool(torch.isnan(t[20:]).all()) and not bool(torch.isnan(t[:20]).any())
        base = t._base
        assert int(torch.isnan(base).sum()) == base.numel() - 20 * segs[s]
    assert torch.equal(torch.cat([t[:20] for t in xs], 1), x[:20])
    ws = G.place_w(w, contiguous=False)
    assert ws.stride(0) == 516 and not ws.is_contiguous() and torch.equal(ws, w) and bool(torch.isnan(ws._base[:, 512:]).all())
    assert G.place_w(w, contiguous=True).is_contiguous()
    for n in (1, 33, 40):
        o = G.place_y(33, n)
        assert o.view.shape == (33, n) and o.buf.stride(0) % 4 == 0 and o.view.storage_offset() == 4
        assert o.buf.shape[0] == 35 and o.buf.shape[1] >= n + 8 and G.outside_intact(o.buf, [])
        o.view.zero_()
        assert G.outside_intact(o.buf, [(33, o.col0, n)]) and not G.outside_intact(o.buf, [(32, o.col0, n)])
