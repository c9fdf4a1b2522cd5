"""The grouped GEMM and LayerNorm kernels (csrc/gemm.hip), linear_f32_mfma (csrc/linear.hip) and rowdot_sigmoid_kernel
(csrc/rowops.hip) against the float64 model of tests/gemm_ref.py at their tile, chunk, segment, m_live and launch-walk edges.

Every GEMM case names the instantiation it reaches (gemm_ref.route_of, proven on the tables by tests/test_gemm_ref_host.py)
and runs among operands placed where a misread does harm: x segments as column slices of NaN-filled buffers with their own
strides and offsets, W with NaN behind each row on the exact routes, NaN in the rows of x at and past m_live, y as a column
slice of a sentinel-filled buffer. Bounds, none of them new (tests/test_split_range.py, tests/test_dense.py):
  (a) finite wherever float64 is;                       (b) |got - want| <= 2e-5 * (|x| . |W|^T + |bias| + flag |bias2|);
  (c) split routes: max err <= 4 e_exact + 1e-7 max magnitude, e_exact the same launch on the exact kernel;
  (d) one-hot x: float32(W[n, k(r)]) + float32(bias[n]) bit for bit on the exact routes; within 2^-21 of the row's
      largest |w| on the split routes (bias off there: one more rounding of a sum is not what the bound is about);
  (e) the sentinel intact around y, rows in [live, M) exactly 0.0;   (f) a row's bits do not depend on its neighbours.
(b) and (c) judge accumulated rounding and are applied to the dense inputs (randn, cancel); a one-hot row has none, and its
statement is (d): on a split route an element of W below the half normals keeps its 22 bits relative to the row, not to
itself. Every figure is printed as `FIG ...` before it is asserted (pytest -s)."""
import ctypes
import itertools

import pytest
import torch

from simpb_amd import _lib
from simpb_amd.plugin import dense, routes
from tests import gemm_ref as G

gpu = pytest.mark.gpu
DEV = "cuda"
ROUTE_NAMES = list(G.ROUTES)
_CACHE = {}


def _fig(*what):
    print("FIG", *what)


def _operands(kind, m, n, k):
    """(x, w, b, b2, (x . W^T, |x| . |W|^T)) for the full extent of a sweep, made and multiplied once."""
    key = (kind, m, n, k)
    if key not in _CACHE:
        x, w, b, b2 = G.gemm_inputs(kind, m, n, k)
        _CACHE[key] = (x, w, b, b2, G.products(x, w))
    return _CACHE[key]


def _spec(x, w, segs, bias=None, relu=False, live=None, flags=None, bias2=None, halfs=False, product=None, extra=None):
    return dict(x=x, w=w, segs=tuple(segs), bias=bias, relu=relu, live=live, flags=flags, bias2=bias2, halfs=halfs,
                product=product, extra=extra)


def _launch(specs, route, split=None):
    """One dense.gemm launch of `specs` on `route` (split: the routes.gemm_split_fp16 to run under; default the route's).
    Asserts that the table's route is the one the rule gives, and bound (e)'s sentinel; returns the outputs on the CPU."""
    r = G.ROUTES[route]
    split = r.split if split is None else split
    dims = [G.job_dims(s["x"].shape[0], s["w"].shape[0], s["segs"]) for s in specs]
    if split == r.split:
        assert G.route_of(dims, split).name == route, (dims, split)
    jobs, outs = [], []
    for s in specs:
        m, n = s["x"].shape[0], s["w"].shape[0]
        xs = G.place_x(s["x"], s["segs"], s["live"], DEV)
        w = G.place_w(s["w"], r.split, DEV)
        assert not r.split or G.in_window(s["w"]), "a weight outside the split window would leave the split route"
        if s["extra"] == "adjacent":
            prev = outs[-1]
            o = G.place_y(m, n, DEV, into=prev.buf, col0=prev.col0 + prev.view.shape[1])
        else:
            wide = s["extra"] == "adjacent_next"
            o = G.place_y(m, n + (s["room"] if wide else 0), DEV)
            if wide:
                o = G.Out(o.buf, o.buf[:m, o.col0:o.col0 + n], o.col0)
        live_t = torch.tensor([s["live"]], dtype=torch.int32, device=DEV) if s["live"] is not None else None
        dev = lambda t: t.to(DEV) if t is not None else None   # noqa: E731
        jobs.append(dense.job(xs, w, dev(s["bias"]), s["relu"], out=o.view, m_live=live_t, row_flag=dev(s["flags"]),
                              bias2=dev(s["bias2"]), split_halfs=s["halfs"]))
        outs.append(o)
    with routes.override(gemm_split_fp16=split):
        dense.gemm(*jobs)
    torch.cuda.synchronize()
    regions = {}
    for o in outs:
        regions.setdefault(id(o.buf), (o.buf, []))[1].append((o.view.shape[0], o.col0, o.view.shape[1]))
    for buf, reg in regions.values():
        assert G.outside_intact(buf, reg), ("sentinel overwritten", route, dims)
    return [o.view.cpu().clone() for o in outs]


def _grouped_specs(case):
    """The specs of a GROUPED case; a job marked "adjacent" writes next to its predecessor, whose buffer gets the room."""
    _, table = G.GROUPED[case]
    specs = []
    for j, (m, n, segs, bias, relu, extra) in enumerate(table):
        x, w, b, b2 = G.gemm_inputs("randn", m, n, sum(segs), key=f"grouped/{case}/{j}")
        flags = ((torch.arange(m) % 3) == 0).int() if extra == "flags" else None
        specs.append(_spec(x, w, segs, b if bias else None, relu, live=0 if extra == "capacity" else None, flags=flags,
                           bias2=b2 if extra == "flags" else None, extra="adjacent" if extra == "adjacent" else None))
        if extra == "adjacent":
            assert specs[-2]["x"].shape[0] == m
            specs[-2]["extra"], specs[-2]["room"] = "adjacent_next", -(-n // 4) * 4
    return specs


def _want(s):
    return G.gemm_ref([s["x"]], s["w"], s["bias"], s["relu"], s["live"], s["flags"], s["bias2"], product=s["product"])


def _judge(tag, got, s, exact=None):
    """(a), (b), the zero rows of (e), and (c) when the exact kernel's output of the same launch is given."""
    want, mag = _want(s)
    m = s["x"].shape[0]
    live = m if s["live"] is None else max(0, min(m, s["live"]))
    assert bool(torch.isfinite(got).all()), (tag, "non-finite", int((~torch.isfinite(got)).sum()))
    assert bool((got[live:] == 0).all()) and not bool(torch.signbit(got[live:]).any()), (tag, "rows past m_live")
    ratio = G.worst_ratio(got, want, mag)
    _fig(*tag, f"err/magnitude {ratio:.3e}")
    assert ratio <= G.REL, (tag, "error / magnitude", ratio)
    if exact is not None and live:
        err = float((got.double() - want).abs().max())
        e_exact = float((exact.double() - want).abs().max())
        allowed = 4 * e_exact + 1e-7 * float(mag.max())
        _fig(*tag, f"err/(4 e_exact + 1e-7 max magnitude) {err / allowed:.3e}")
        assert err <= allowed, (tag, err, e_exact)
    return ratio


def _judge_onehot(tag, got, s, kidx, split):
    """(d): x row r = e_k(r)."""
    w, b = s["w"], s["bias"]
    assert bool(torch.isfinite(got).all()), (tag, "non-finite")
    col = w[:, kidx].t()
    if not split:
        want = col + b if b is not None else col
        if s["relu"]:
            want = want.clamp_min(0)
        assert torch.equal(got, want), (tag, "placement", int((got != want).sum()), (got != want).nonzero()[:4].tolist())
        return 0.0
    assert b is None
    want = col.double().clamp_min(0) if s["relu"] else col.double()
    ratio = float(((got.double() - want).abs() / w.double().abs().amax(1)[None, :]).max())
    _fig(*tag, f"placement err / row max |w| {ratio:.3e}")
    assert ratio <= G.PLACE_SPLIT, (tag, ratio)
    return ratio


def _run_dense(tag, route, kind, m, n, segs, bias, relu, full):
    """A dense (randn / cancel) case cut from the sweep's operands `full`."""
    x, w, b, _, (p, a) = full
    s = _spec(x[:m], w[:n], segs, b[:n] if bias else None, relu, product=(p[:m, :n], a[:m, :n]))
    got, = _launch([s], route)
    exact = _launch([s], route, split=False)[0] if G.ROUTES[route].split else None
    _judge(tag, got, s, exact)


def _run_onehot(tag, route, m, n, segs, bias, relu, w, b, shifts):
    k = sum(segs)
    split = G.ROUTES[route].split
    for shift in shifts:
        s = _spec(G.onehot_rows(m, k, shift), w[:n], segs, b[:n] if bias and not split else None, relu)
        got, = _launch([s], route)
        _judge_onehot(tag + (f"shift {shift}",), got, s, G.onehot_k(m, k, shift), split)


# ============================================================================================ 1. tile and chunk sweep
@gpu
@pytest.mark.parametrize("kind", ["randn", "cancel", "onehot_x"])
@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_tile_sweep_vs_float64(route, kind):
    """The M x N set of the route (one below / at / one above a row and a column tile, a partial tile) at one K."""
    t = G.SWEEP[route]
    k = sum(t["segs"])
    full = _operands("randn" if kind == "onehot_x" else kind, max(t["ms"]), max(t["ns"]), k)
    for i, (m, n, segs, bias, relu) in enumerate(G.sweep_cases(route)):
        tag = ("sweep", route, kind, f"{m}x{n}x{k}")
        if kind == "onehot_x":
            _run_onehot(tag, route, m, n, segs, bias, relu, full[1], full[2], [(37 * i) % k])
        else:
            _run_dense(tag, route, kind, m, n, segs, bias, relu, full)


@gpu
@pytest.mark.parametrize("kind", ["randn", "cancel", "onehot_x"])
@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_chunk_count_sweep_vs_float64(route, kind):
    """Every chunk count of the route's list (heads and tails of k_loop) at one ragged M x N; the one-hot rows walk every
    k of every chunk."""
    for m, n, segs, bias, relu in G.chunk_cases(route):
        k = sum(segs)
        tag = ("chunks", route, kind, f"{m}x{n}x{k}")
        full = _operands("randn" if kind == "onehot_x" else kind, m, n, k)
        if kind == "onehot_x":
            _run_onehot(tag, route, m, n, segs, bias, relu, full[1], full[2], G.onehot_shifts(m, k))
        else:
            _run_dense(tag, route, kind, m, n, segs, bias, relu, full)


# ============================================================================================ 2. segment boundaries
@gpu
@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_segment_boundaries_vs_float64(route):
    """K = 256 and 512 cut into 1-4 segments every way the route admits, each segment in its own buffer with its own stride
    and offset: the one-hot rows pin that chunk c comes from the right segment at the right column."""
    m, n = G.SEGMENT_SHAPE[route]
    for segs in G.segment_cases(route):
        k = sum(segs)
        full = _operands("randn", m, n, k)
        tag = ("segments", route, "x".join(map(str, segs)))
        _run_onehot(tag + ("onehot_x",), route, m, n, segs, True, False, full[1], full[2], G.onehot_shifts(m, k))
        _run_dense(tag + ("randn",), route, "randn", m, n, segs, True, False, full)
    # one-hot rows of W: column n of y is column k(n) of x
    segs = G.segment_cases(route)[-1]
    k = sum(segs)
    x, _, b, _ = G.gemm_inputs("randn", m, n, k)
    for shift in G.onehot_shifts(n, k):
        s = _spec(x, G.onehot_rows(n, k, shift), segs, None if G.ROUTES[route].split else b)
        got, = _launch([s], route)
        col = x[:, G.onehot_k(n, k, shift)]
        if G.ROUTES[route].split:
            ratio = float(((got.double() - col.double()).abs() / x.double().abs().amax(1, keepdim=True)).max())
            _fig("segments", route, "onehot_w", f"placement err / row max |x| {ratio:.3e}")
            assert ratio <= G.PLACE_SPLIT
        else:
            assert torch.equal(got, col + b), ("onehot_w", route, shift)


# ============================================================================================ 3. m_live
@gpu
@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_m_live_edges_vs_float64(route):
    """live in {0, 1, tile - 1, tile, tile + 1, M - 1, M, M + 5} on a ragged M of three or more row tiles, NaN in every row
    of x at and past live: zeros there, and the surviving rows bit for bit those of the full launch."""
    t = G.SWEEP[route]
    m, n = t["ragged"]
    full = _operands("randn", m, n, sum(t["segs"]))
    x, w, b, _, product = full
    base = _spec(x, w, t["segs"], b, False, product=product)
    whole, = _launch([base], route)
    _judge(("m_live", route, "no m_live"), whole, base)
    for live in G.live_values(route):
        s = dict(base, live=live)
        got, = _launch([s], route)
        _judge(("m_live", route, f"live {live}"), got, s)
        rows = min(live, m)
        assert torch.equal(got[:rows], whole[:rows]), ("rows below m_live differ from the full launch", route, live)


# ============================================================================================ 4. grouped launches
@gpu
@pytest.mark.parametrize("case", list(G.GROUPED))
def test_grouped_launch_vs_float64(case):
    """1-4 jobs of different M, N, K, segments and epilogues in one launch; totals of tiles with remainders 0, 1 and 7
    modulo 8 (surplus workgroups return), a job of capacity rows only between live ones, two jobs writing adjacent column
    ranges of one buffer. Every job comes out as it does alone (where it alone stays on the route) or with the jobs in the
    reverse order (other tile_start values), bit for bit."""
    route = G.GROUPED[case][0]
    specs = _grouped_specs(case)
    split = G.ROUTES[route].split
    outs = _launch(specs, route)
    exact = _launch(specs, route, split=False) if split else [None] * len(specs)
    _fig("grouped", case, route, "tiles", G.total_tiles(G.grouped_dims(case), split))
    for j, (s, got) in enumerate(zip(specs, outs)):
        _judge(("grouped", case, route, f"job {j}"), got, s, exact[j])
        alone_spec = dict(s, extra=None)
        dims = [G.job_dims(s["x"].shape[0], s["w"].shape[0], s["segs"])]
        if G.route_of(dims, split).name == route:
            alone, = _launch([alone_spec], route)
            assert torch.equal(got, alone), ("grouped != alone", case, j)
    if len(specs) > 1:
        rev = [dict(s, extra=None) for s in reversed(specs)]
        for j, (got, other) in enumerate(zip(outs, reversed(_launch(rev, route)))):
            assert torch.equal(got, other), ("grouped != reversed order", case, j)


# ============================================================================================ 5. epilogue forms at edges
def _edge_flags(m, tile):
    f = (torch.arange(m) % 2).int()
    for r, v in ((tile - 1, 1), (tile, 0), (2 * tile - 1, 0), (2 * tile, 1), (m - 1, 1)):
        f[r] = v
    return f


@gpu
@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_epilogue_forms_at_edges_vs_float64(route):
    """row_flag + bias2 (flags alternating, and set / clear on both sides of the row-tile borders), relu and the half-pair
    output on the ragged shape of each route."""
    t = G.SWEEP[route]
    m, n = t["ragged"]
    x, w, b, b2, product = _operands("randn", m, n, sum(t["segs"]))
    flags = _edge_flags(m, G.ROUTES[route].tile_m)
    split = G.ROUTES[route].split
    for relu, live in ((False, None), (True, None), (True, m - 3)):
        s = _spec(x, w, t["segs"], b, relu, live=live, flags=flags, bias2=b2, product=product)
        got, = _launch([s], route)
        exact = _launch([s], route, split=False)[0] if split else None
        _judge(("epilogue", route, f"flags relu={relu} live={live}"), got, s, exact)
        packed, = _launch([dict(s, halfs=True)], route)
        words = packed.view(torch.int32)
        rows = m if live is None else live
        assert bool((words[rows:] == 0).all()), ("half-pair words past m_live are not all-zero bits", route)
        dec = G.halfs_value(words[:rows])
        y = got[:rows].double()
        ratio = float(((dec - y).abs() / y.abs().clamp_min(G.HALF_MIN_NORMAL)).max())
        _fig("epilogue", route, f"half pairs relu={relu} live={live}", f"err / max(|y|, 2^-14) {ratio:.3e}")
        assert ratio <= G.PLACE_SPLIT, (route, ratio)   # two halfs carry 22 bits of a normal half's leading part
        assert bool((dec[y == 0] == 0).all())


# ============================================================================================ 6. second-pass rows
@gpu
@pytest.mark.parametrize("route", list(G.SPLIT_ROUTES))
def test_second_pass_rows_vs_float64(route):
    """One row scaled by 2^20 (outside the split window): first, last and in the middle of a row tile, and in the partial
    last tile next to the clamped rows. Its tile takes the second pass; every other row keeps its bits."""
    t = G.SWEEP[route]
    m, n = t["ragged"]
    tm = G.ROUTES[route].tile_m
    x, w, b, _, _ = _operands("randn", m, n, sum(t["segs"]))
    base, = _launch([_spec(x, w, t["segs"], b)], route)
    assert m % tm, "the last row tile is partial"
    for row in (0, tm - 1, tm + tm // 2, m - 1):
        xb = G.big_row(x, row)
        s = _spec(xb, w, t["segs"], b)
        got, = _launch([s], route)
        exact, = _launch([s], route, split=False)
        _judge(("second pass", route, f"row {row}"), got, s, exact)
        others = torch.arange(m) != row
        assert torch.equal(got[others], base[others]), ("a neighbour of the out-of-window row changed", route, row)


# ============================================================================================ (f) row independence
@gpu
@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_row_bits_do_not_depend_on_position(route):
    """The rows of x rolled by 13 (every row in another lane, most in another tile) give the rolled output; on the routes
    that a one-row launch stays on, single rows alone give their rows of the full launch."""
    t = G.SWEEP[route]
    m, n = t["ragged"]
    x, w, b, _, _ = _operands("randn", m, n, sum(t["segs"]))
    base, = _launch([_spec(x, w, t["segs"], b)], route)
    rolled, = _launch([_spec(torch.roll(x, 13, 0), w, t["segs"], b)], route)
    assert torch.equal(torch.roll(rolled, -13, 0), base), route
    split = G.ROUTES[route].split
    if G.route_of([G.job_dims(1, n, t["segs"])], split).name == route:
        for row in (0, 31, 32, m - 1):
            one, = _launch([_spec(x[row:row + 1], w, t["segs"], b)], route)
            assert torch.equal(one[0], base[row]), (route, row)


# ============================================================================================ 7. layernorm_seg_kernel
def _place_ln(x, k0, k1, live):
    xs = G.place_x(x, (k0, k1) if k1 else (k0,), live, DEV)
    o = G.place_y(x.shape[0], k0 + k1, DEV)
    return xs, o


def _ln_module(g, b):
    ln = torch.nn.LayerNorm(g.numel()).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(g)
        ln.bias.copy_(b)
    return ln


@gpu
@pytest.mark.parametrize("kind", G.LN_KINDS)
@pytest.mark.parametrize("k0,k1", G.LN_WIDTHS)
def test_layernorm_edges_vs_float64(k0, k1, kind):
    """Rows 1, 3, 4, 5, 301 (a workgroup is four rows), two segments of different strides, m_live at the row edges.
    randn: absolute 2e-5. offset / const / tiny: at most 4x the error of the float32 evaluation of the same formula plus
    1e-7 of the largest magnitude. Rows past live are zeros, the sentinel around y is intact, and a row's bits are those
    it has in the 301-row launch."""
    d = k0 + k1
    xf, g, b = G.ln_inputs(kind, max(G.LN_ROWS), d)
    want_f, mag_f = G.layernorm_ref([xf], g, b)
    e32 = float((G.layernorm_f32([xf], g, b).double() - want_f).abs().max())
    allowed = G.LN_ABS if kind == "randn" else 4 * e32 + 1e-7 * float(mag_f.max())
    ln = _ln_module(g, b)
    whole, worst = None, 0.0
    for rows in reversed(G.LN_ROWS):
        for live in [None] + G.rows_live_values(rows):
            xs, o = _place_ln(xf[:rows], k0, k1, live)
            live_t = torch.tensor([live], dtype=torch.int32, device=DEV) if live is not None else None
            dense.layernorm(xs, ln, out=o.view, m_live=live_t)
            torch.cuda.synchronize()
            got = o.view.cpu()
            assert G.outside_intact(o.buf, [(rows, o.col0, d)]), ("sentinel", rows, live)
            n_live = rows if live is None else min(rows, live)
            assert bool((got[n_live:] == 0).all()) and bool(torch.isfinite(got).all()), (rows, live)
            if whole is None:
                whole = got.clone()
            assert torch.equal(got[:n_live], whole[:n_live]), ("row bits depend on the launch", rows, live)
            worst = max(worst, float((got[:n_live].double() - want_f[:n_live]).abs().max()) if n_live else 0.0)
    _fig("layernorm", f"{k0}+{k1}", kind, f"err {worst:.3e} e32 {e32:.3e} allowed {allowed:.3e} ratio {worst / allowed:.3e}")
    assert worst <= allowed, (k0, k1, kind, worst, e32)


@gpu
def test_layernorm_refusals():
    x = torch.zeros(4, 576, device=DEV)
    with pytest.raises(RuntimeError, match="SIMPB_EINVAL"):
        dense.layernorm(x, torch.nn.LayerNorm(576).to(DEV))
    with pytest.raises(ValueError, match="eps"):
        dense.layernorm(x[:, :512], torch.nn.LayerNorm(512, eps=1e-6).to(DEV))
    torch.cuda.synchronize()


# ============================================================================================ 8. linear_f32_mfma
def _linear_f32_into(ybuf, x, w, b, m, n, k, relu):
    from simpb_amd.plugin.ops import _stream
    return _lib.lib().simpb_linear_f32(ybuf.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None,
                                       m, n, k, 1 if relu else 0, _stream())


def _in_nan(t):
    """A contiguous copy of t on the device with NaN before it (16 bytes) and behind it."""
    flat = torch.full((t.numel() + 8,), float("nan"))
    flat[4:4 + t.numel()] = t.reshape(-1)
    return flat.to(DEV)[4:4 + t.numel()].view(t.shape)


@gpu
def test_linear_f32_tile_edges_vs_float64():
    """M in {1, 63, 64, 65, 129} x N in {1, 255, 256, 257, 513} x K in {32, 64, 96} (the 64 x 256 tile, chunks of 32):
    randn under (a) and (b), one-hot x under (d), bias and relu in their four forms, two sentinel rows behind row M."""
    from simpb_amd.plugin.ops import linear_f32
    forms = list(itertools.product((True, False), (False, True)))
    worst = 0.0
    for i, (m, n, k) in enumerate(itertools.product(G.LINEAR_M, G.LINEAR_N, G.LINEAR_K)):
        bias, relu = forms[i % 4]
        x, w, b, _ = G.gemm_inputs("randn", m, n, k, key="linear")
        bd = b.to(DEV) if bias else None
        wd = _in_nan(w)
        for kind, shifts in (("randn", (0,)), ("onehot_x", G.onehot_shifts(m, k))):
            for shift in shifts:
                xc = x if kind == "randn" else G.onehot_rows(m, k, shift)
                ybuf = torch.full((m + 2, n), G.SENTINEL, device=DEV)
                assert _linear_f32_into(ybuf, _in_nan(xc), wd, bd, m, n, k, relu) == 0
                torch.cuda.synchronize()
                got = ybuf.cpu()
                assert bool((got[m:] == G.SENTINEL).all()), ("rows past M written", m, n, k)
                got = got[:m]
                assert bool(torch.isfinite(got).all()), (m, n, k, kind)
                if kind == "randn":
                    want, mag = G.gemm_ref([xc], w, b if bias else None, relu)
                    ratio = G.worst_ratio(got, want, mag)
                    worst = max(worst, ratio)
                    assert ratio <= G.REL, (m, n, k, ratio)
                    assert torch.equal(linear_f32(xc.to(DEV), w.to(DEV), bd, relu).cpu(), got)
                else:
                    want = w[:, G.onehot_k(m, k, shift)].t()
                    want = want + b if bias else want
                    assert torch.equal(got, want.clamp_min(0) if relu else want), ("placement", m, n, k, shift)
    _fig("linear_f32", f"worst err/magnitude {worst:.3e}")


@gpu
def test_linear_f32_refusals():
    from simpb_amd.plugin.ops import linear_f32
    x, w = torch.zeros(8, 48, device=DEV), torch.zeros(16, 48, device=DEV)
    with pytest.raises(ValueError, match="K % 32"):
        linear_f32(x, w)
    ybuf = torch.full((8, 16), G.SENTINEL, device=DEV)
    assert _linear_f32_into(ybuf, x, w, None, 8, 16, 48, False) == 1
    flat = torch.zeros(8 * 64 + 1, device=DEV)
    w64 = torch.zeros(16, 64, device=DEV)
    with pytest.raises(RuntimeError, match="SIMPB_EINVAL"):
        linear_f32(flat[1:].view(8, 64), w64)   # x 4 bytes off a 16-byte boundary
    assert _linear_f32_into(ybuf, flat[1:], w64, None, 8, 16, 64, False) == 1
    torch.cuda.synchronize()
    assert bool((ybuf == G.SENTINEL).all())


# ============================================================================================ 9. rowdot_sigmoid_kernel
@gpu
@pytest.mark.parametrize("k", G.ROWDOT_K)
def test_rowdot_sigmoid_edges_vs_float64(k):
    """x a strided slice among NaN, rows around the four of a workgroup, m_live at the row edges, the bias driving the
    logits to +-100: the sigmoid saturates (exactly 1 above; below 1e-30 and finite below) without NaN."""
    worst = 0.0
    xf, w, _, _ = G.gemm_inputs("randn", max(G.ROWDOT_ROWS), 1, k, key="rowdot")
    wd = w.to(DEV)
    for rows, bias in itertools.product(G.ROWDOT_ROWS, (0.3, 100.0, -100.0)):
        b = torch.tensor([bias])
        for live in [None] + G.rows_live_values(rows):
            xs, = G.place_x(xf[:rows], (k,), live, DEV)
            assert xs.stride(0) == k + 8 and xs.storage_offset() == 4
            live_t = torch.tensor([live], dtype=torch.int32, device=DEV) if live is not None else None
            got = dense.rowdot_sigmoid(xs, wd, b.to(DEV), m_live=live_t).cpu()
            want = G.rowdot_sigmoid_ref(xf[:rows], w, b, live)
            assert got.shape == (rows, 1) and bool(torch.isfinite(got).all()), (k, rows, bias, live)
            n_live = rows if live is None else min(rows, live)
            assert bool((got[n_live:] == 0).all())
            err = float((got.double() - want).abs().max())
            worst = max(worst, err)
            assert err <= G.ROWDOT_ABS, (k, rows, bias, live, err)
            if bias == 100.0:
                assert bool((got[:n_live] == 1).all())
            if bias == -100.0:
                assert bool((got[:n_live] < 1e-30).all())
    _fig("rowdot_sigmoid", f"k {k}", f"worst err {worst:.3e}")


@gpu
def test_rowdot_sigmoid_refuses_k_6():
    with pytest.raises(RuntimeError, match="SIMPB_EINVAL"):
        dense.rowdot_sigmoid(torch.zeros(4, 6, device=DEV), torch.zeros(6, device=DEV), torch.zeros(1, device=DEV))
    torch.cuda.synchronize()


# ============================================================================================ 10. host rejections
@gpu
def test_gemm_host_rejections():
    """simpb_gemm_f32 through ctypes: each malformed launch returns SIMPB_EINVAL and writes nothing."""
    from simpb_amd.plugin.ops import _stream
    m, n, k = 8, 16, 128
    x = torch.zeros(m + 1, k + 8, device=DEV)
    w = torch.zeros(n + 1, k + 8, device=DEV)
    y = torch.full((m, n + 4), G.SENTINEL, device=DEV)
    aux = torch.zeros(64, device=DEV)
    flag = torch.zeros(m, dtype=torch.int32, device=DEV)

    def args(num_jobs=1, **over):
        a = dense._Args()
        a.num_jobs = num_jobs
        for j in range(min(max(num_jobs, 1), dense.MAX_JOBS)):
            jb = a.job[j]
            jb.x[0], jb.ldx[0], jb.kseg[0] = x.data_ptr(), k + 8, k
            jb.num_seg, jb.M, jb.N, jb.K = 1, m, n, k
            jb.w, jb.ldw, jb.y, jb.ldy = w.data_ptr(), k + 8, y.data_ptr(), n + 4
            for name, value in over.items():
                if name in ("x", "ldx", "kseg"):
                    for s, v in enumerate(value):
                        getattr(jb, name)[s] = v
                else:
                    setattr(jb, name, value)
        return a

    def call(a):
        return _lib.lib().simpb_gemm_f32(ctypes.byref(a), _stream())

    assert call(args()) == 0   # the well-formed launch these cases are edits of
    torch.cuda.synchronize()
    assert bool((y[:, :n] == 0).all()) and bool((y[:, n:] == G.SENTINEL).all())
    y.fill_(G.SENTINEL)
    bad = {
        "num_jobs 0": args(0), "num_jobs 5": args(5),
        "K % 64": args(K=96, kseg=[96]),
        "sum kseg != K": args(kseg=[64]),
        "sum kseg != K (two segments)": args(num_seg=2, kseg=[64, 128], x=[x.data_ptr()] * 2, ldx=[k + 8] * 2),
        "ldy < N": args(ldy=n - 1),
        "ldx < kseg": args(ldx=[k - 4]),
        "ldx % 4": args(ldx=[k + 6]),
        "x misaligned": args(x=[x.data_ptr() + 4]),
        "w misaligned": args(w=w.data_ptr() + 8),
        "row_flag without bias2": args(row_flag=flag.data_ptr()),
        "bias2 without row_flag": args(bias2=aux.data_ptr()),
    }
    for name, a in bad.items():
        assert call(a) == 1, name
    torch.cuda.synchronize()
    assert bool((y == G.SENTINEL).all())
