"""Range of the split-operand FP16 kernels against float64.

x = xh + xl / 2^11 carries 22 bits only inside a window of magnitudes: |x| >= 65520 makes xh infinite, and a row far below
2^-14 loses its trailing bits to half subnormals. The GEMM kernels (csrc/gemm.hip gemm_f16x3_kernel / _wide_kernel) and
linear_split's linear_f16x3_kernel stage a row of x whose largest |x| lies outside [2^-10, 2^15) as x * 2^-e and scale
the sum back in the epilogue; a weight with a row outside that window takes the exact-fp32 kernel (dense.split_in_window),
which the tests assert. Bounds have no absolute floor:
  * per element |got - want| <= 2e-5 * (|x| @ |W|^T + |b|), in float64;
  * at most 4x the error of the exact-fp32 kernel on the same operands, plus 1e-7 of the largest such magnitude;
  * finite wherever float64 is.
Scaling x (or W) and b by 2^s scales the float64 result by exactly 2^s, so one reference serves a whole sweep.
The attention kernels still need |q|, |k|, |v| < 65504: their out-of-range cases are strict xfails that pin the limit."""
import math

import pytest
import torch

from simpb_amd import synth
from simpb_amd.plugin import dense

gpu = pytest.mark.gpu
SCALES = (-40, -30, -20, -10, 0, 10, 16, 17, 20, 40)


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("s", SCALES)
def test_split_in_window_matches_float64_reconstruction(s):
    """The host check accepts exactly the weights whose rows' largest |w| lie in the window, and on those the two-half
    split reconstructs every element to 2^-21 of its row's largest |w| (float64)."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(64, 256, generator=g) / 16 * 2.0 ** s
    rowmax = w.double().abs().amax(1)
    inside = bool(((rowmax >= 2.0 ** -10) & (rowmax < 2.0 ** 15)).all())
    assert dense.split_in_window(w) == inside
    if inside:
        hi = w.half()
        lo = ((w - hi.float()) * 2048.0).half()
        rec = hi.double() + lo.double() / 2048.0
        assert bool(torch.isfinite(rec).all())
        assert float(((rec - w.double()).abs() / rowmax[:, None]).max()) <= 2.0 ** -21


def test_split_in_window_row_cases():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(8, 128, generator=g) / 12
    assert dense.split_in_window(w)
    z = w.clone()
    z[2] = 0   # an all-zero row needs no exponent
    assert dense.split_in_window(z)
    for value in (1e5, 1e-9, float("inf"), float("nan")):
        bad = w.clone()
        bad[5] = w[5] / w[5].abs().max() * value if math.isfinite(value) else value
        assert not dense.split_in_window(bad), value
    edge = w.clone()
    edge[1] = edge[1] / edge[1].abs().max() * 2.0 ** 15   # the window is half open
    assert not dense.split_in_window(edge)
    edge[1] = edge[1] / 2
    assert dense.split_in_window(edge)


# ---------------------------------------------------------------------------------------------------- GPU
SHAPES = {
    "narrow32": (900, 256, (512, 256, 256), False),   # 32-wide tiles, 128-deep chunks, three segments
    "narrow64": (900, 1536, (256, 256), False),       # 64-wide tiles (the q|k|v projection)
    "ragged4seg": (65, 70, (128, 128, 128, 128), True),
    "one_chunk": (33, 100, (128,), False),
    "wide": (2250, 1536, (256, 256), False),          # 64 x 128 tiles, partial last row tile
    "wide_ragged_n": (3300, 1000, (512,), True),      # 64 x 128 tiles, partial column tiles
}
_CACHE = {}


def _operands(name):
    if name not in _CACHE:
        m, n, ks, relu = SHAPES[name]
        g = torch.Generator().manual_seed(m * 7 + n)
        xs = [torch.randn(m, k, generator=g) for k in ks]
        w = torch.randn(n, sum(ks), generator=g) / math.sqrt(sum(ks))
        b = torch.randn(n, generator=g)
        _CACHE[name] = (xs, w, b, relu) + _ref(xs, w, b, relu)
    return _CACHE[name]


def _ref(xs, w, b, relu):
    x = torch.cat([t.double() for t in xs], -1)
    want = x @ w.double().t()
    mag = x.abs() @ w.double().abs().t()
    if b is not None:
        want, mag = want + b.double(), mag + b.double().abs()
    return (want.clamp_min(0) if relu else want), mag


def _run(xs, w, b, relu):
    from simpb_amd.plugin import routes
    args = ([x.cuda() for x in xs], w.cuda(), b.cuda() if b is not None else None)
    got = dense.linear(*args, relu=relu).cpu()
    with routes.override(gemm_split_fp16=False):
        exact = dense.linear(*args, relu=relu).cpu()
    return got, exact


def _check(got, exact, want, mag, what):
    assert bool(torch.isfinite(got).all()), (what, "non-finite output", int((~torch.isfinite(got)).sum()))
    err = (got.double() - want).abs()
    worst = float((err / mag.clamp_min(1e-300)).max())
    assert bool((err <= 2e-5 * mag).all()), (what, "error / (|x|@|W|^T + |b|)", worst)
    e_exact = float((exact.double() - want).abs().max())
    assert float(err.max()) <= 4 * e_exact + 1e-7 * float(mag.max()), (what, float(err.max()), e_exact)


def _assert_route(w, split):
    """Which GEMM kernel a launch with this weight takes: the split one exactly when the weight is inside the window."""
    w_hi, _ = dense._split_weights(w.cuda().contiguous())
    assert (w_hi is not None) == split


@gpu
@pytest.mark.parametrize("side", ["x", "w"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_gemm_power_of_two_sweep_vs_float64(name, s, side):
    """Side x: x * 2^s and b * 2^s on the split kernel (W stays inside the window). Side w: W * 2^s and b * 2^s; the split
    kernel while W is inside the window, the exact one outside it. The float64 result scales by exactly 2^s."""
    xs, w, b, relu, want, mag = _operands(name)
    f = 2.0 ** s
    if side == "x":
        xs, w_s = [x * f for x in xs], w
        _assert_route(w_s, True)
    else:
        w_s = w * f
        rowmax = w_s.double().abs().amax(1)
        _assert_route(w_s, bool(((rowmax >= 2.0 ** -10) & (rowmax < 2.0 ** 15)).all()))
    got, exact = _run(xs, w_s, b * f, relu)
    _check(got, exact, want * f, mag * f, (name, side, s))


def _mixed(case, xs, w):
    xs = [x.clone() for x in xs]
    w = w.clone()
    if case == "x_outlier_1e6":
        xs[-1][5, 17] = 1e6
    elif case == "x_row_1e-9":
        for x in xs:
            x[7] *= 1e-9
    elif case == "x_zero_rows":
        for x in xs:
            x[10:42] = 0
    elif case == "w_row_1e5":
        w[3] *= 1e5 / float(w[3].abs().max())
    elif case == "w_row_1e-9":
        w[3] *= 1e-9
    return xs, w


@gpu
@pytest.mark.parametrize("case", ["x_outlier_1e6", "x_row_1e-9", "x_zero_rows", "w_row_1e5", "w_row_1e-9"])
@pytest.mark.parametrize("name", ["narrow32", "narrow64", "ragged4seg", "wide"])
def test_gemm_mixed_magnitudes_vs_float64(name, case):
    """One row or element out of range among unit values, no bias (so the bound of a 1e-9 row is its own product): only
    that row takes the second pass; a weight row out of range sends the launch to the exact kernel."""
    xs, w, _, relu, _, _ = _operands(name)
    xs, w = _mixed(case, xs, w)
    _assert_route(w, not case.startswith("w_"))
    want, mag = _ref(xs, w, None, relu)
    got, exact = _run(xs, w, None, relu)
    _check(got, exact, want, mag, (name, case))


@gpu
def test_gemm_out_of_range_rows_with_m_live():
    """Capacity rows past *m_live stay zeros while a live row needs the second pass."""
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 700, 256, generator=g)
    x[0, 3] *= 2.0 ** 20
    w = torch.randn(384, 256, generator=g) / 16
    b = torch.randn(384, generator=g)
    live = torch.tensor([411], dtype=torch.int32, device="cuda")
    got = dense.linear(x.cuda(), w.cuda(), b.cuda(), m_live=live).cpu()
    want, mag = _ref([x[0, :411]], w, b, False)
    assert bool(torch.isfinite(got).all()) and bool((got[0, 411:] == 0).all())
    assert bool(((got[0, :411].double() - want).abs() <= 2e-5 * mag).all())


@gpu
def test_head_with_feature_maps_past_the_half_range_vs_oracle(monkeypatch):
    """(Every weight of the product head stays on the split path: the spy counts only jobs that take the split kernel.)
    The product head against the oracle on feature maps scaled by the smallest power of two that pushes an input of a
    split GEMM (the deformable aggregation's output into output_proj) above 2^16: one cold and one warm frame, the
    oracle tolerance of tests/test_gpu_head.py, every output finite. A spy on dense.gemm checks that the range is
    reached, so the test cannot silently stop exercising it."""
    from oracle import simpb_ref as R
    from simpb_amd.plugin import ops
    from tests.helpers import build_product_head, load_golden, metas_to, spec_of
    spec = spec_of(load_golden("head_small.npz"))
    seen = []
    orig = dense.gemm

    def spy(*jobs):
        for j in jobs:   # inputs of jobs that take the split kernel: 128-aligned segments and a weight inside the window
            w = j["w"]
            if (all(x.shape[-1] % 128 == 0 for x in j["xs"]) and w.dtype == torch.float32 and w.is_contiguous()
                    and dense._split_weights(w)[0] is not None):
                seen.extend(float(x.abs().max()) for x in j["xs"] if x.numel())
        return orig(*jobs)
    monkeypatch.setattr(dense, "gemm", spy)

    def frame(head, f, scale):
        maps = synth.feature_maps_nchw(spec["bs"], f, spec["image_wh"], seed=9, scale=scale)
        metas = synth.frame_metas(spec["bs"], f, spec["image_wh"])
        return maps, metas, head(ops.feature_maps_format([x.cuda() for x in maps]), metas_to(metas, "cuda"))

    with torch.no_grad():
        probe = build_product_head(spec)
        for k in range(8, 30):
            seen.clear()
            frame(probe, 0, 2.0 ** k)
            if max(seen) > 2.0 ** 16:
                break
        assert max(seen) > 2.0 ** 16, "no split-GEMM input above 2^16"
        del probe
        head = build_product_head(spec)
        params = {n: v.detach().cpu() for n, v in head.state_dict().items()}
        oracle = R.OracleHead(params, head.operation_order, spec["num_anchor"], spec["num_temp"], spec["num_output"])
        for f in range(2):
            seen.clear()
            maps, metas, got = frame(head, f, 2.0 ** k)
            assert max(seen) > 2.0 ** 16, (f, max(seen))
            want = oracle.forward(R.feature_maps_format(maps), metas)
            for name in ("prediction", "classification", "quality", "prediction2d", "classification2d"):
                for a, b in zip(got[name], want[name]):
                    if b is None:
                        assert a is None
                        continue
                    assert bool(torch.isfinite(a).all()), (name, f, k)
                    assert float((a.cpu() - b).abs().max()) <= 1e-3, (name, f, k)


# ---------------------------------------------------------------------------------------------------- linear_split
def _lin_case(m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / 16, torch.randn(n, generator=g)


@gpu
@pytest.mark.parametrize("side", ["x", "w"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("m,n,k", [(1000, 256, 256), (77, 40, 192)])
def test_linear_split_power_of_two_sweep_vs_float64(m, n, k, s, side):
    """linear_f16x3_kernel (f32 x): x * 2^s or W * 2^s, with b * 2^s, against float64 and the exact linear_f32."""
    from simpb_amd.plugin.ops import linear_f32, linear_split
    x, w, b = _lin_case(m, n, k, m + n)
    want, mag = _ref([x], w, b, False)
    f = 2.0 ** s
    x, w = (x * f, w) if side == "x" else (x, w * f)
    got = linear_split(x.cuda(), w.cuda(), (b * f).cuda()).cpu()
    exact = linear_f32(x.cuda(), w.cuda(), (b * f).cuda()).cpu()
    _check(got, exact, want * f, mag * f, ("linear_split", side, s))


@gpu
@pytest.mark.parametrize("case", ["x_outlier_1e6", "x_row_1e-9", "w_row_1e5", "w_row_1e-9"])
def test_linear_split_mixed_magnitudes_vs_float64(case):
    from simpb_amd.plugin.ops import linear_f32, linear_split
    x, w, _ = _lin_case(1000, 256, 256, 5)
    (x,), w = _mixed(case, [x], w)
    want, mag = _ref([x], w, None, False)
    got = linear_split(x.cuda(), w.cuda()).cpu()
    exact = linear_f32(x.cuda(), w.cuda()).cpu()
    _check(got, exact, want, mag, ("linear_split", case))


@gpu
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("m,n,k", [(1000, 256, 256), (130, 72, 64)])
def test_linear_split_f16_input_weight_sweep_vs_float64(m, n, k, s):
    """linear_h2_kernel (x already f16: exact as given): W * 2^s and b * 2^s; outside the window the exact kernel."""
    from simpb_amd.plugin.ops import linear_f32, linear_split
    x, w, b = _lin_case(m, n, k, m + k)
    x = x.half()
    f = 2.0 ** s
    want, mag = _ref([x.float()], w * f, b * f, False)
    got = linear_split(x.cuda(), (w * f).cuda(), (b * f).cuda()).cpu()
    exact = linear_f32(x.float().cuda(), (w * f).cuda(), (b * f).cuda()).cpu()
    _check(got, exact, want, mag, ("linear_h2", s))


# ---------------------------------------------------------------------------------------------------- attention
# (a, b): q * 2^a with k * 2^-a leaves S unchanged; v * 2^b scales O by exactly 2^b. The kernels have no range handling
# yet: beyond the half range they return NaN. Those cases are strict xfails, so the limit cannot change unnoticed.
ATT_OK = [(0, 0), (10, 0), (-10, 0), (0, 10), (0, -10)]
ATT_LIMIT = [(20, 0), (-20, 0), (0, 20)]
ATT_CASES = [pytest.param(a, b, id=f"a{a}_b{b}") for a, b in ATT_OK] + [
    pytest.param(a, b, id=f"a{a}_b{b}", marks=pytest.mark.xfail(strict=True, reason="attention operands beyond the half range"))
    for a, b in ATT_LIMIT]
_BOUNDS = [0, 40, 40, 77, 100, 131, 140]   # camera groups of 150 slots: group 1 empty, 140.. capacity pads


def _att_ref(q, k, v, grouped):
    n = q.shape[1]
    qd, kd, vd = (t.double().reshape(1, n, 8, 64).transpose(1, 2) for t in (q, k, v))
    s = qd @ kd.transpose(-1, -2)
    if grouped:
        mask = torch.full((n, n), float("-inf"), dtype=torch.float64)
        for c in range(6):
            mask[_BOUNDS[c]:_BOUNDS[c + 1], _BOUNDS[c]:_BOUNDS[c + 1]] = 0
        s = s + mask
    p = torch.nan_to_num(torch.softmax(s, -1))
    return ((p @ vd).transpose(1, 2).reshape(1, n, 512), (p @ vd.abs()).transpose(1, 2).reshape(1, n, 512))


@gpu
@pytest.mark.parametrize("a,b", ATT_CASES)
@pytest.mark.parametrize("form", ["f16s", "halfs", "halfs_grouped"])
def test_attention_split_power_of_two_vs_float64(form, a, b):
    """attention_f16s_kernel (split=1, fp32 operands) and the shipped chain: the q|k|v GEMM with split_halfs output (softmax
    scale folded into the q rows, plugin/layers.py:173-189) into attention_halfs_kernel, plain and camera-grouped."""
    from simpb_amd.plugin.ops import attention_f32
    g = torch.Generator().manual_seed(21)
    n = 150 if form == "halfs_grouped" else 300
    x = torch.randn(1, n, 512, generator=g)
    w = torch.randn(1536, 512, generator=g) / math.sqrt(512)
    bias = torch.randn(1536, generator=g) * 0.1
    rs = torch.cat([torch.full((512,), 0.125 * 2.0 ** a), torch.full((512,), 2.0 ** -a), torch.full((512,), 2.0 ** b)])
    w, bias = w * rs[:, None], bias * rs
    qkv64 = x[0].double() @ w.double().t() + bias.double()
    q, k, v = (qkv64[None, :, i * 512:(i + 1) * 512] for i in range(3))
    grouped = form == "halfs_grouped"
    want, mag = _att_ref(q, k, v, grouped)
    tables = ()
    if grouped:
        cam = torch.full((n,), -1, dtype=torch.int32)
        for c in range(6):
            cam[_BOUNDS[c]:_BOUNDS[c + 1]] = c
        tables = (cam.cuda(), torch.tensor(_BOUNDS, dtype=torch.int32).cuda())
    q32, k32, v32 = (t.float().cuda() for t in (q * 8.0, k, v))   # the unscaled q for the kernels that scale it
    exact = attention_f32(q32, k32, v32, 8, *tables, split=0).cpu()
    if form == "f16s":
        got = attention_f32(q32, k32, v32, 8, split=1).cpu()
    else:
        packed = dense.linear(x.cuda(), w.cuda(), bias.cuda(), split_halfs=True)
        got = attention_f32(packed[..., :512], packed[..., 512:1024], packed[..., 1024:], 8, *tables, split=2).cpu()
    _check(got, exact, want, mag, (form, a, b))
