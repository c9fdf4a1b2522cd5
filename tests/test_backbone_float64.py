"""The fp16 backbone's convolution kernels against their float64 statement (tests/conv_ref.py) at tile and map edges.

Kernels: conv3x3_f16_kernel<AF, KSPLIT> (variants 1-4), conv_staged_kernel (variants 5-8 and the 1x1 tilings 2-3),
conv_staged_group_kernel, the TOK16 forms (csrc/conv3x3.hip); conv1x1_f16_kernel (csrc/conv1x1.hip); stem_conv_pool_kernel and
image_to_nhwc4_kernel (csrc/stem.hip); bias_act_nhwc_f16_kernel and bias_relu_maxpool_kernel (csrc/bias_act.hip), each through
its entry in plugin/ops.py. The reference is float64 on the CPU; no vendor convolution is called.

Bounds (no absolute floor beyond the f16 subnormal quantum):
  (e) per element  |got - want| <= sum over rounding points max(2^-11 |v|, 2^-25) + KAPPA * 2^-24 * abs_sum   (conv_ref.bound_e);
  (x) on one-hot inputs every output equals the f16 value float64 gives; bias_act / bias_relu_maxpool equal f16(float64)
      wherever fp32 evaluates the expression exactly (equality of values: a zero's sign is not compared);
  (o) |want| >= 2^16 * 1.01 -> +-inf of the right sign; |want| <= 65504 * 0.99 -> finite and within (e); under 1 % between;
  (a) no NaN, documented shape / dtype / layout, sentinels around every output and in every foreign token row intact, inputs
      embedded in NaN-filled storage.
KAPPA is twice what two float32 references need on the same cases (torch's conv2d in float32, and a float32 sum in the
kernels' order: tap by tap, 64 channels per chunk); test_fp32_reference_stays_under_half_of_the_bounds measures it.

Inputs (seeded f16 values): `randn`; `cancel` (outputs about three orders below abs_sum); `small` (activations and bias
* 2^-12: f16 subnormal operands and results); `big` (a clear share of outputs past 2^16); `onehot0/1` (one 1.0 per image at a
corner, an edge or the interior, on a channel in the second half of the last 64-chunk; integer weights coded from
(cout, tap, cin), integer bias and residual: every fp32 sum is exact and an output names the tap and channel read).
Each test prints its figures (`FIG ...`) before it asserts."""
import functools
import math
import zlib

import pytest
import torch

from tests import conv_ref as R

gpu = pytest.mark.gpu

# What the float32 references need over every GPU case of this module (test_fp32_reference_stays_under_half_of_the_bounds):
# see KAPPA_SET_BY. KAPPA is twice the largest figure, rounded up. "Needs" = the smallest kappa with
# |ref - want| <= rounding terms + kappa * 2^-24 * abs_sum: a reference that rounds its result to f16 uses the rounding terms
# in full, so it is the kappa term of (e) of which the references stay under half.
KAPPA = 9.0
KAPPA_SET_BY = "4.31: conv2d in float32 on conv1x1 512 -> 192, map (3, 9, 13), stride 2, `cancel` with residual; kernels' order: 2.74"

F64 = torch.float64
SENT, PAD = -1237.0, 1024          # an f16 value; elements of padding on either side of a buffer (a multiple of 8: 16 bytes)

DEGENERATE = [(1, 1, 1), (2, 1, 7), (2, 7, 1), (3, 3, 3)]
ODD = [(3, 5, 7), (3, 9, 13)]
AROUND = {32: [(1, 1, 31), (2, 4, 4), (1, 3, 11)], 64: [(1, 7, 9), (1, 8, 8), (1, 5, 13)], 96: [(1, 5, 19), (2, 6, 8), (1, 1, 97)],
          128: [(1, 1, 127), (1, 8, 16), (1, 3, 43)], 256: [(1, 15, 17), (1, 16, 16), (1, 1, 257)]}
ALL_KINDS = ("randn", "cancel", "small", "big", "onehot0", "onehot1")


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def ints(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float()


def hot_place(i, k, h, w):
    """Where image i's single 1.0 sits under one-hot kind k: (bottom-right corner = the last pixel of the image | left edge
    | interior | bottom edge | top edge | right edge | top-left corner); three images and two kinds reach the first six."""
    order = [(h - 1, w - 1), (h // 2, 0), (h // 2, w // 2), (h - 1, w // 2), (0, w // 2), (h // 2, w - 1), (0, 0)]
    return order[(2 * i + k) % 7]


def coded_weights(cout, kh, kw, cin):
    """Integers in [-1019, 1019] from (cout, tap, cin): neighbouring taps, channels and filters all differ."""
    co = torch.arange(cout).view(-1, 1, 1)
    tap = torch.arange(kh * kw).view(1, -1, 1)
    ci = torch.arange(cin).view(1, 1, -1)
    return (((37 * ci + 229 * tap + 11 * co) % 2039) - 1019).float().reshape(cout, kh, kw, cin)


def onehot_map(n, h, w, c, k, channel):
    x = torch.zeros(n, h, w, c)
    for i in range(n):
        y0, x0 = hot_place(i, k, h, w)
        x[i, y0, x0, channel(i)] = 1.0
    return x


def h16(t):
    return t.to(torch.float16)


# ------------------------------------------------------------------------------------------------------------- conv3x3
CPAIRS3 = [(64, 8), (64, 72), (128, 64), (192, 136), (256, 192)]
TILE3 = {1: (128, 64), 2: (256, 64), 3: (32, 64), 4: (64, 64), 5: (128, 64), 6: (128, 128), 7: (96, 64), 8: (96, 128)}
# (variant, map, channel pair): tile counts 7 and 17 on the direct (variants 1-4) and the staged (5-8) launch path, which no
# natural case reaches (1, 8 and 9 occur on both: profiles/backbone_convs_vs_float64.md)
EXTRA3 = [(3, (1, 14, 16), (64, 8)), (3, (1, 23, 23), (64, 8)), (7, (1, 23, 27), (64, 8)), (7, (1, 39, 41), (64, 8))]
# variant 0 at the smallest maps on which it chooses variant 4, 1, 7 and 8 (everything smaller runs variant 3)
SELECT3 = [((1, 64, 64), (64, 72), 4), ((1, 64, 128), (64, 72), 1), ((1, 96, 128), (64, 72), 7), ((1, 80, 96), (192, 136), 8)]


def chosen3(p_out, cout):
    """simpb_conv3x3_nhwc_f16's choice for variant 0, restated."""
    t96, t128, t64, ny = -(-p_out // 96), -(-p_out // 128), -(-p_out // 64), -(-cout // 64)
    n128 = -(-cout // 128)
    if cout >= 128 and t128 * n128 >= 2048:
        return 6
    if cout >= 128 and t96 * n128 >= 160:
        return 8
    if t96 * ny >= 256:
        return 7
    if t128 * ny >= 128:
        return 1
    if t64 * ny >= 128:
        return 4
    return 3


def tiles3(variant, p_out, cout):
    bm, bn = TILE3[variant]
    return -(-p_out // bm) * -(-cout // bn)


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def cases3(variant):
    """(map, stride, (cin, cout), kind) of a forced variant, or of variant 0 (which runs variant 3 on all of them)."""
    own = AROUND[TILE3[variant or 3][0]]
    out = []
    for cp in CPAIRS3:
        for m in DEGENERATE + ODD + own:
            for stride in (1, 2):
                kinds = ALL_KINDS if m in ODD else ("randn", "onehot0", "onehot1")
                out += [(m, stride, cp, kind) for kind in kinds]
    out += [(m, 1, cp, kind) for v, m, cp in EXTRA3 if v == variant for kind in ("randn", "onehot0", "onehot1")]
    if variant == 0:
        out += [(m, 1, cp, "randn") for m, cp, _ in SELECT3]
    return out


@functools.lru_cache(maxsize=None)
def case3(m, stride, cp, kind):
    """Operands (f16, NHWC) and the float64 statement before the ReLU."""
    n, h, w = m
    cin, cout = cp
    g = torch.Generator().manual_seed(seed_of("c3", m, stride, cp, kind))
    k = 9 * cin
    x, wt, b = randn(g, n, h, w, cin), randn(g, cout, 3, 3, cin) / math.sqrt(k), randn(g, cout)
    if kind == "cancel":      # a nearly constant map: the output is the bias against a sum a thousand times larger
        x = 1 + x / 64
        conv = R.conv_taps(h16(x), h16(wt), stride, 1)
        inner = conv[:, 1:-1, 1:-1] if min(conv.shape[1:3]) > 2 else conv
        b = -inner.mean((0, 1, 2)).float()
    elif kind == "small":
        x, b = x * 2.0 ** -12, b * 2.0 ** -12
    elif kind == "big":
        x, wt, b = x * 2.0 ** 8, wt * 2.0 ** 7, b * 2.0 ** 10
    elif kind.startswith("onehot"):
        kk = int(kind[-1])
        x = onehot_map(n, h, w, cin, kk, lambda i: cin - 32 + (5 * i + 3 * kk) % 32)
        wt, b = coded_weights(cout, 3, 3, cin), ints(g, cout)
    x, wt, b = h16(x), h16(wt), h16(b)
    return dict(x=x, w=wt, b=b, pre=R.conv3x3(x, wt, b, stride, relu=False))


def with_relu(ref, relu):
    return R.Ref(ref.want.clamp_min(0), ref.abs_sum, ref.extra) if relu else ref


# ------------------------------------------------------------------------------------------------------------- conv1x1
CIN1 = (64, 128, 192, 256, 512, 576)
COUT1 = (8, 72, 136, 192)
MAPS1 = DEGENERATE + ODD + AROUND[128]
UP_MAPS = [(2, 2, 2), (3, 4, 6), (1, 8, 16)]
INB_MAPS = [(3, 5, 7)] + AROUND[128]


def cases1(cin):
    """(map, stride, cin, cout, kind, form) with form in plain | res | up | inb | inb_res."""
    out = []
    for cout in COUT1:
        for m in MAPS1:
            for stride in (1, 2):
                for form in ("plain", "res"):
                    kinds = ("randn", "onehot0")
                    if m in ODD:
                        kinds = ALL_KINDS[:5] if form == "res" else ("randn", "small", "big", "onehot0")
                    out += [(m, stride, cin, cout, kind, form) for kind in kinds]
        out += [(m, 1, cin, cout, kind, "up") for m in UP_MAPS for kind in ("randn", "onehot0", "onehot1")]
        for m in INB_MAPS:
            for form in ("inb", "inb_res"):
                kinds = ("randn", "small", "onehot0") if m in ODD else ("randn", "onehot0")
                out += [(m, 1, cin, cout, kind, form) for kind in kinds]
    return out


@functools.lru_cache(maxsize=None)
def case1(m, stride, cin, cout, kind, form):
    n, h, w = m
    ho, wo = out_hw(h, w, stride)
    g = torch.Generator().manual_seed(seed_of("c1", m, stride, cin, cout, kind, form))
    x, wt, b = randn(g, n, h, w, cin), randn(g, cout, cin) / math.sqrt(cin), randn(g, cout)
    rshape = (n, ho // 2, wo // 2, cout) if form == "up" else (n, ho, wo, cout)
    res = randn(g, *rshape) if form in ("res", "up", "inb_res") else None
    inb = randn(g, cin) if form.startswith("inb") else None
    if kind == "small":
        x, b = x * 2.0 ** -12, b * 2.0 ** -12
        res = res * 2.0 ** -12 if res is not None else None
        inb = inb * 2.0 ** -12 if inb is not None else None
    elif kind == "big":
        x, wt, b = x * 2.0 ** 8, wt * 2.0 ** 7, b * 2.0 ** 10
        res = res * 2.0 ** 12 if res is not None else None
    elif kind.startswith("onehot"):
        kk = int(kind[-1])
        x = onehot_map(n, h, w, cin, kk, lambda i: cin - 32 + (5 * i + 3 * kk) % 32)
        wt, b = coded_weights(cout, 1, 1, cin).reshape(cout, cin), ints(g, cout)
        if form == "up":      # one element per residual image: an output names the residual pixel that was read
            res = 7 * onehot_map(n, ho // 2, wo // 2, cout, 1 - kk, lambda i: (3 * i + 5) % cout)
        elif res is not None:
            res = ints(g, *rshape)
        if inb is not None:
            inb = torch.randint(-2, 3, (cin,), generator=g).float()
    x, wt, b = h16(x), h16(wt), h16(b)
    res = h16(res) if res is not None else None
    inb = h16(inb) if inb is not None else None
    if kind == "cancel":      # the residual takes the rounded result away: what is left is its rounding residue
        res = h16(-R.conv1x1(x, wt, b, None, False, stride).want)
    pre = R.conv1x1(x, wt, b, res, False, stride, form == "up", inb)
    return dict(x=x, w=wt, b=b, res=res, inb=inb, pre=pre)


# ---------------------------------------------------------------------------------------------------------------- stem
STEM_IMAGES = [(1, 1, 1), (2, 3, 5), (1, 7, 9), (2, 31, 63), (2, 32, 64), (1, 33, 65), (1, 34, 66), (3, 69, 37)]
STEM_KINDS = ("randn", "small", "big", "onehot0")


@functools.lru_cache(maxsize=None)
def case_stem(m, kind):
    n, h, w = m
    g = torch.Generator().manual_seed(seed_of("stem", m, kind))
    img, wt, b = randn(g, n, h, w, 3), randn(g, 64, 7, 7, 3) / math.sqrt(147), randn(g, 64)
    if kind == "small":
        img, b = img * 2.0 ** -12, b * 2.0 ** -12
    elif kind == "big":
        img, wt = img * 2.0 ** 8, wt * 2.0 ** 6.5      # the pooled maximum of nine: 2 % past 2^16
    elif kind == "onehot0":
        img = onehot_map(n, h, w, 3, 0, lambda i: i % 3)
        wt, b = coded_weights(64, 7, 7, 3), ints(g, 64)
    img, wt, b = h16(img), h16(wt), h16(b)
    return dict(img=img, w=wt, b=b, ref=R.stem(img, wt, b))


# -------------------------------------------------------------------------------------------- bias_act, bias_relu_maxpool
EPI_C = (8, 24, 64)
EPI_MAPS = [(1, 1, 1), (3, 6, 5), (2, 7, 9)]
EPI_KINDS = ("randn", "small", "big")
WRAP = (1, 513, 512, 64)      # 2 101 248 pieces of 8 against the 8 192 x 256 = 2 097 152 threads of the capped grid


@functools.lru_cache(maxsize=4)
def case_epi(m, c, kind):
    n, h, w = m
    g = torch.Generator().manual_seed(seed_of("epi", m, c, kind))
    scale = {"randn": 1.0, "small": 2.0 ** -12, "big": 2.0 ** 14}[kind]
    return dict(y=h16(randn(g, n, h, w, c) * scale), b=h16(randn(g, c) * scale), res=h16(randn(g, n, h, w, c) * scale))


def fp32_exact(*terms):
    """Elements on which the fp32 sum of `terms` (in order) is exact at every step."""
    acc32, acc64 = terms[0].float(), terms[0].to(F64)
    ok = torch.ones_like(acc64, dtype=torch.bool)
    for t in terms[1:]:
        acc32, acc64 = acc32 + t.float(), acc64 + t.to(F64)
        ok &= acc32.to(F64) == acc64
    return ok


# ---------------------------------------------------------------------------------------------------------- judging
class Tally:
    """Figures and failures of one test: printed first, asserted afterwards."""

    def __init__(self, name):
        self.name, self.figs, self.notes, self.failures = name, {}, [], []
        self.band, self.big = 0, 0          # elements of `big` cases in the unjudged overflow band / in all

    def fig(self, label, value):
        self.figs[label] = max(self.figs.get(label, 0.0), value)

    def note(self, text):
        self.notes.append(text)

    def fail(self, *what):
        self.failures.append(" ".join(str(w) for w in what))

    def finish(self):
        for text in self.notes:
            print(f"FIG {self.name} {text}")
        for label, value in sorted(self.figs.items()):
            print(f"FIG {self.name} {label} = {value:.3f}")
        if self.big:
            print(f"FIG {self.name} unjudged overflow band: {self.band} of {self.big} elements = {self.band / self.big:.4f}")
            if self.band >= 0.01 * self.big:
                self.fail("unjudged overflow band", self.band / self.big)
        assert not self.failures, (len(self.failures), self.failures[:8])


def judge(t, where, got, ref, kind, label):
    """(e), (x), (o) and the NaN part of (a) for one output (NHWC, on the CPU)."""
    g = got.to(F64)
    want = ref.want
    if tuple(g.shape) != tuple(want.shape):
        return t.fail(where, "shape", tuple(g.shape), tuple(want.shape))
    if bool(torch.isnan(g).any()):
        t.fail(where, "NaN in the output")
    hi, lo = want.abs() >= 2.0 ** 16 * 1.01, want.abs() <= R.F16_MAX * 0.99
    band = int((~(hi | lo)).sum())
    if kind == "big":
        t.band, t.big = t.band + band, t.big + want.numel()
    elif band:
        t.fail(where, "an output in the unjudged band of a case that is not `big`")
    if not bool((g[hi] == torch.sign(want[hi]) * float("inf")).all()):
        t.fail(where, "(o) not +-inf past 2^16")
    if not bool(torch.isfinite(g[lo]).all()):
        t.fail(where, "(o) inf below 65504")
    e = R.figure_e(got, ref, KAPPA, lo)
    t.fig(f"{label} {kind[:6]} e", e)
    t.fig(f"{label} {kind[:6]} kappa", R.kappa_needed(got, ref))      # what the kernel needs of the kappa term (of KAPPA)
    if not e <= 1.0:
        t.fail(where, "bound (e)", e)
    if kind.startswith("onehot") and not bool((g == want.to(torch.float16).to(F64)).all()):
        t.fail(where, "(x) one-hot output differs from f16(float64)")


# ------------------------------------------------------------------------------------------ device buffers with sentinels
def embed(t, fill=float("nan")):
    """A contiguous CUDA copy of t inside `fill`-filled storage; (tensor, whole buffer)."""
    n = t.numel()
    whole = torch.full((n + 2 * PAD,), fill, dtype=t.dtype, device="cuda")
    inner = whole[PAD:PAD + n].view(t.shape)
    inner.copy_(t)
    return inner, whole


def dev(t):
    return None if t is None else embed(t)[0]


def nchw(t):
    """NHWC storage as the channels_last [N, C, H, W] tensor the operators take."""
    return None if t is None else t.permute(0, 3, 1, 2)


def nhwc_cpu(t):
    return t.permute(0, 2, 3, 1).cpu()


def pads_intact(whole, n, fill=SENT):
    pad = torch.cat([whole[:PAD], whole[PAD + n:]])
    return bool(torch.isnan(pad).all()) if fill != fill else bool((pad == fill).all())


class _GuardedTorch:
    """Stands in for `torch` inside plugin/ops.py: every tensor the operators allocate lies inside a sentinel-filled buffer
    and holds the sentinel itself where torch.empty is asked for (channels_last included)."""

    def __init__(self):
        self.buffers = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, fill, *shape, **kw):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        n = math.prod(shape)
        whole = torch.full((n + 2 * PAD,), SENT, dtype=kw.get("dtype") or torch.float32, device=kw["device"])
        flat = whole[PAD:PAD + n]
        if kw.get("memory_format") is torch.channels_last:
            inner = flat.view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)
        else:
            inner = flat.view(shape)
        if fill is not None:
            inner.fill_(fill)
        self.buffers.append((whole, n))
        return inner

    def empty(self, *shape, **kw):
        return self._alloc(None, *shape, **kw)

    def zeros(self, *shape, **kw):
        return self._alloc(0.0, *shape, **kw)

    def problems(self, out):
        """After a launch: `out` lies in a guarded buffer and every buffer's padding holds the sentinel."""
        torch.cuda.synchronize()
        bad = []
        if out is not None and not any(w.data_ptr() + PAD * w.element_size() == out.data_ptr() for w, _ in self.buffers):
            bad.append("the output was allocated outside the guarded buffers")
        if not all(pads_intact(w, n) for w, n in self.buffers):
            bad.append("write outside an output")
        self.buffers = []
        return bad


@pytest.fixture
def guard():
    from simpb_amd.plugin import ops
    real, g = ops.torch, _GuardedTorch()
    ops.torch = g
    try:
        yield g
    finally:
        ops.torch = real


def layout_problems(y, shape):
    bad = []
    if tuple(y.shape) != tuple(shape) or y.dtype != torch.float16:
        bad.append(f"shape / dtype {tuple(y.shape)} {y.dtype}")
    elif not y.is_contiguous(memory_format=torch.channels_last):
        bad.append("not channels_last")
    return bad


@functools.lru_cache(maxsize=None)
def dev3(key):
    c = case3(*key)
    return nchw(dev(c["x"])), nchw(dev(c["w"])), dev(c["b"])


@functools.lru_cache(maxsize=None)
def dev1(key):
    c = case1(*key)
    cout, cin = c["w"].shape
    return nchw(dev(c["x"])), dev(c["w"]).view(cout, cin, 1, 1), dev(c["b"]), nchw(dev(c["res"])), dev(c["inb"])


# ============================================================================================== GPU: conv3x3, map output
@gpu
@pytest.mark.parametrize("cp", CPAIRS3, ids=lambda cp: f"{cp[0]}to{cp[1]}")
@pytest.mark.parametrize("variant", range(9))
def test_conv3x3_vs_float64(variant, cp, guard):
    from simpb_amd.plugin.ops import conv3x3_nhwc
    t = Tally(f"conv3x3 v{variant} {cp[0]}->{cp[1]}")
    counts = set()
    for key in [k for k in cases3(variant) if k[2] == cp]:
        m, stride, _, kind = key
        c = case3(*key)
        x, w, b = dev3(key)
        ho, wo = out_hw(m[1], m[2], stride)
        p_out = m[0] * ho * wo
        ran = variant or chosen3(p_out, cp[1])
        counts.add(tiles3(ran, p_out, cp[1]))
        if variant == 0 and kind == "randn":
            t.note(f"map {m} stride {stride}: variant 0 runs {ran}, {tiles3(ran, p_out, cp[1])} tiles")
        for relu in ((False, True) if not kind.startswith("onehot") else (False,)):
            where = (m, stride, kind, relu)
            y = conv3x3_nhwc(x, w, b, relu=relu, stride=stride, variant=variant)
            for p in guard.problems(y) + layout_problems(y, (m[0], cp[1], ho, wo)):
                t.fail(where, p)
            judge(t, where, nhwc_cpu(y), with_relu(c["pre"], relu), kind, "map")
    t.note(f"tile counts {sorted(counts)}")
    if variant == 0:
        for m, scp, expect in SELECT3:
            if scp == cp and chosen3(m[0] * m[1] * m[2], cp[1]) != expect:
                t.fail("variant 0 selection", m, expect)
    t.finish()


# ============================================================================================ GPU: conv3x3, token output
TOK_MAP = (6, 3, 5)
TOK_BS, TOK_CAMS = 2, 3
PYRAMID = [(4, 11), (2, 6), (1, 3), (1, 1)]


def token_buffers(bs, rows, c, f32):
    """Sentinel-filled token buffers inside sentinel padding: (f32 [bs, rows, c] or None, f16, wholes)."""
    shape = torch.Size((bs, rows, c))
    t16, w16 = embed(torch.full(shape, SENT, dtype=torch.float16), SENT)
    t32, w32 = embed(torch.full(shape, SENT, dtype=torch.float32), SENT) if f32 else (None, None)
    return t32, t16, [w for w in (w16, w32) if w is not None]


def judge_tokens(t, where, t32, t16, wholes, refs, starts, per_cam, kind):
    """Rows against the reference's own layout; foreign rows and padding hold the sentinel; f32 rows = the f16 rows widened."""
    torch.cuda.synchronize()
    n = t16.numel()
    if not all(pads_intact(w, n) for w in wholes):
        t.fail(where, "write outside the token buffer")
    want, written = R.token_rows([r.want for r in refs], TOK_BS, TOK_CAMS, per_cam, starts)
    ab, _ = R.token_rows([r.abs_sum for r in refs], TOK_BS, TOK_CAMS, per_cam, starts)
    ex, _ = R.token_rows([r.extra for r in refs], TOK_BS, TOK_CAMS, per_cam, starts)
    got = t16.cpu()
    if not bool((got[~written] == SENT).all()):
        t.fail(where, "a row of another level or past the level's rows was written (f16)")
    if t32 is not None:
        g32 = t32.cpu()
        if not bool((g32[~written] == SENT).all()):
            t.fail(where, "a row of another level or past the level's rows was written (f32)")
        if not torch.equal(g32[written], got[written].float()):
            t.fail(where, "f32 rows are not the f16 rows widened")
    judge(t, where, got[written], R.Ref(want[written], ab[written], ex[written]), kind, "tokens")


@gpu
@pytest.mark.parametrize("f32", [True, False], ids=["f32_and_f16", "f16_alone"])
@pytest.mark.parametrize("variant", [3, 7, 8])
def test_conv3x3_token_rows_vs_float64(variant, f32):
    from simpb_amd.plugin.ops import conv3x3_nhwc
    t = Tally(f"conv3x3 tokens v{variant} {'f32+f16' if f32 else 'f16'}")
    per_cam, start = 3 * 5 + 9, 4           # level_start > 0, tokens_per_cam larger than the level
    for cp in ((64, 72), (128, 64)):
        for kind in ("randn", "onehot0", "onehot1"):
            key = (TOK_MAP, 1, cp, kind)
            c = case3(*key)
            x, w, b = dev3(key)
            t32, t16, wholes = token_buffers(TOK_BS, TOK_CAMS * per_cam, cp[1], f32)
            out = conv3x3_nhwc(x, w, b, relu=False, stride=1, tokens=(t32, per_cam, start, t16), variant=variant)
            if out is not None:
                t.fail(cp, kind, "token form returned a tensor")
            judge_tokens(t, (cp, kind), t32, t16, wholes, [c["pre"]], [start], per_cam, kind)
    t.finish()


@gpu
@pytest.mark.parametrize("f32", [True, False], ids=["f32_and_f16", "f16_alone"])
@pytest.mark.parametrize("cp", [(256, 256), (64, 72)], ids=["256to256", "64to72"])
@pytest.mark.parametrize("levels", [1, 2, 4])
def test_conv3x3_group_token_rows_vs_float64(levels, cp, f32):
    from simpb_amd.plugin.ops import conv3x3_group_tokens
    t = Tally(f"conv3x3 group {levels} levels {cp[0]}->{cp[1]} {'f32+f16' if f32 else 'f16'}")
    pyr = PYRAMID[:levels]
    starts, at = [], 3                      # level_start > 0, a gap of two rows between levels, five spare rows behind
    for h, w in pyr:
        starts.append(at)
        at += h * w + 2
    per_cam = at + 5
    n = TOK_BS * TOK_CAMS
    for kind in ("randn", "onehot0", "onehot1"):
        keys = [((n, h, w), 1, cp, kind) for h, w in pyr]
        cs = [case3(*k) for k in keys]
        ds = [dev3(k) for k in keys]
        t32, t16, wholes = token_buffers(TOK_BS, TOK_CAMS * per_cam, cp[1], f32)
        conv3x3_group_tokens([d[0] for d in ds], [d[1] for d in ds], [d[2] for d in ds], t32, per_cam, starts, col16=t16)
        judge_tokens(t, kind, t32, t16, wholes, [c["pre"] for c in cs], starts, per_cam, kind)
    t.note(f"tiles {[tiles3(8, n * h * w, cp[1]) for h, w in pyr]}")
    t.finish()


# ============================================================================================================ GPU: conv1x1
def chosen1(cin, form):
    return 1 if form.startswith("inb") or cin < 512 else 2


@gpu
@pytest.mark.parametrize("cin", CIN1)
@pytest.mark.parametrize("variant", range(4))
def test_conv1x1_vs_float64(variant, cin, guard):
    from simpb_amd.plugin.ops import conv1x1_nhwc
    t = Tally(f"conv1x1 v{variant} cin{cin}")
    for key in cases1(cin):
        m, stride, _, cout, kind, form = key
        if form.startswith("inb") and variant > 1:
            continue                        # rejected by the host: test_conv1x1_host_rejections
        c = case1(*key)
        x, w, b, res, inb = dev1(key)
        ho, wo = out_hw(m[1], m[2], stride)
        for relu in ((False, True) if not kind.startswith("onehot") else (False,)):
            where = (m, stride, cout, kind, form, relu)
            y = conv1x1_nhwc(x, w, b, residual=res, relu=relu, stride=stride, residual_upsample2x=form == "up", input_bias=inb,
                             variant=variant)
            for p in guard.problems(y) + layout_problems(y, (m[0], cout, ho, wo)):
                t.fail(where, p)
            judge(t, where, nhwc_cpu(y), with_relu(c["pre"], relu), kind, form)
    if variant == 0:
        t.note(f"variant 0 runs {chosen1(cin, 'plain')} (with input_bias: 1)")
    t.finish()


@gpu
def test_conv1x1_host_rejections():
    from simpb_amd.plugin.ops import conv1x1_nhwc
    key = ((3, 5, 7), 1, 64, 8, "randn", "inb_res")
    x, w, b, res, inb = dev1(key)
    for variant in (2, 3):
        with pytest.raises(RuntimeError, match="SIMPB_EINVAL"):
            conv1x1_nhwc(x, w, b, residual=res, input_bias=inb, variant=variant)
    for m in ((3, 5, 7), (1, 4, 7), (1, 5, 4)):        # an odd output height or width
        small = torch.zeros(m[0], 8, m[1] // 2, m[2] // 2, dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last)
        xm = torch.zeros(m[0], 64, m[1], m[2], dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last)
        with pytest.raises(ValueError, match="even output sizes"):
            conv1x1_nhwc(xm, w, b, residual=small, residual_upsample2x=True)
    with pytest.raises(ValueError, match="needs a residual"):
        conv1x1_nhwc(x, w, b, residual=None, residual_upsample2x=True)
    torch.cuda.synchronize()


# =============================================================================================================== GPU: stem
@gpu
@pytest.mark.parametrize("kind", STEM_KINDS)
@pytest.mark.parametrize("m", STEM_IMAGES, ids=lambda m: "x".join(map(str, m)))
def test_stem_vs_float64(m, kind, guard):
    from simpb_amd.plugin.ops import stem_conv_pool, stem_conv_pool_nhwc4
    t = Tally(f"stem {m} {kind}")
    c = case_stem(m, kind)
    n, h, w = m
    hp, wp = out_hw(*out_hw(h, w, 2), 2)
    wt, b = dev(c["w"]).permute(0, 3, 1, 2), dev(c["b"])
    img = c["img"].float().permute(0, 3, 1, 2).contiguous()                    # f32 [N, 3, H, W] holding f16 values
    wide = torch.full((n, 5, h, w + 3), float("nan"))
    wide[:, 1:4, :, 2:w + 2] = img
    x4 = torch.zeros(n, h, w, 4, dtype=torch.float16)
    x4[..., :3] = c["img"]
    routes = {"image": lambda: stem_conv_pool(dev(img), wt, b),
              "strided view": lambda: stem_conv_pool(dev(wide)[:, 1:4, :, 2:w + 2], wt, b),
              "nhwc4": lambda: stem_conv_pool_nhwc4(dev(x4), wt, b)}
    for name, run in routes.items():
        y = run()
        for p in guard.problems(y) + layout_problems(y, (n, 64, hp, wp)):
            t.fail(name, p)
        judge(t, name, nhwc_cpu(y), c["ref"], kind, "pooled")
    t.finish()


# ======================================================================================== GPU: bias_act_, bias_relu_maxpool
def judge_exact(t, where, got, ref, exact):
    g = got.to(F64)
    t.fig("fp32-exact share", float(exact.double().mean()))
    if not bool((g[exact] == ref.want[exact].to(torch.float16).to(F64)).all()):
        t.fail(where, "(x) differs from f16(float64) where fp32 is exact")


@gpu
@pytest.mark.parametrize("kind", EPI_KINDS)
@pytest.mark.parametrize("c", EPI_C)
def test_bias_act_vs_float64(c, kind):
    from simpb_amd.plugin.ops import bias_act_
    t = Tally(f"bias_act C{c} {kind}")
    for m in EPI_MAPS:
        d = case_epi(m, c, kind)
        for relu in (False, True):
            for with_res in (False, True):
                res = d["res"] if with_res else None
                y, whole = embed(d["y"])
                out = bias_act_(nchw(y), dev(d["b"]), nchw(dev(res)), relu=relu)
                torch.cuda.synchronize()
                where = (m, relu, with_res)
                if out.data_ptr() != y.data_ptr() or not pads_intact(whole, y.numel(), float("nan")):
                    t.fail(where, "not in place, or a write outside the map")
                ref = R.bias_act(d["y"], d["b"], res, relu)
                judge(t, where, y.cpu(), ref, kind, "map")
                if kind == "randn":
                    terms = [d["y"], d["b"].expand_as(d["y"])] + ([res] if with_res else [])
                    judge_exact(t, where, y.cpu(), ref, fp32_exact(*terms))
    t.finish()


@gpu
def test_bias_act_past_the_grid_stride_wrap():
    """(1, 64, 513, 512): 2 101 248 pieces of 8 against the 2 097 152 threads of the capped grid; the last 4 096 pieces are a
    thread's second trip."""
    from simpb_amd.plugin.ops import bias_act_
    t = Tally("bias_act wrap")
    g = torch.Generator().manual_seed(seed_of("wrap"))
    y0, b, res = h16(randn(g, *WRAP)), h16(randn(g, WRAP[3])), h16(randn(g, *WRAP))
    y, whole = embed(y0)
    bias_act_(nchw(y), dev(b), nchw(dev(res)), relu=True)
    torch.cuda.synchronize()
    if not pads_intact(whole, y.numel(), float("nan")):
        t.fail("a write outside the map")
    ref = R.bias_act(y0, b, res, True)
    judge(t, "wrap", y.cpu(), ref, "randn", "map")
    judge_exact(t, "wrap", y.cpu(), ref, fp32_exact(y0, b.expand_as(y0), res))
    t.finish()


@gpu
@pytest.mark.parametrize("kind", EPI_KINDS)
@pytest.mark.parametrize("c", EPI_C)
def test_bias_relu_maxpool_vs_float64(c, kind, guard):
    from simpb_amd.plugin.ops import bias_relu_maxpool
    t = Tally(f"bias_relu_maxpool C{c} {kind}")
    for m in EPI_MAPS:
        d = case_epi(m, c, kind)
        y = bias_relu_maxpool(nchw(dev(d["y"])), dev(d["b"]))
        hp, wp = out_hw(m[1], m[2], 2)
        for p in guard.problems(y) + layout_problems(y, (m[0], c, hp, wp)):
            t.fail(m, p)
        ref = R.bias_relu_maxpool(d["y"], d["b"])
        judge(t, m, nhwc_cpu(y), ref, kind, "pooled")
        if kind == "randn":
            exact = R.max_pool((~fp32_exact(d["y"], d["b"].expand_as(d["y"]))).double(), 0.0) == 0.0   # the whole window
            judge_exact(t, m, nhwc_cpu(y), ref, exact)
    t.finish()


# ================================================================================================ non-GPU: the reference
def test_reference_agrees_with_torch_float64_operators():
    """conv_ref's tap-by-tap statement against torch's own float64 conv2d / max_pool2d / interpolate, and its token layout
    against a permute-and-concatenate restatement."""
    import torch.nn.functional as F
    for key in [((3, 9, 13), 2, (128, 64), "randn"), ((2, 1, 7), 1, (64, 72), "randn"), ((3, 5, 7), 2, (64, 8), "cancel")]:
        c = case3(*key)
        want = R.conv_torch(c["x"], c["w"], key[1], 1, F64) + c["b"].to(F64)
        assert float((c["pre"].want - want).abs().max()) <= 1e-12 * float(c["pre"].abs_sum.max())
        assert bool((c["pre"].abs_sum >= c["pre"].want.abs() * (1 - 1e-12)).all())
    c = case1((3, 4, 6), 1, 128, 72, "randn", "up")
    want = F.conv2d(nchw(c["x"]).double(), c["w"].double().view(72, 128, 1, 1), c["b"].double())
    want = want + F.interpolate(nchw(c["res"]).double(), scale_factor=2, mode="nearest")
    assert float((nchw(c["pre"].want) - want).abs().max()) <= 1e-12 * float(c["pre"].abs_sum.max())
    c = case1((3, 9, 13), 2, 64, 8, "randn", "plain")
    want = F.conv2d(nchw(c["x"]).double(), c["w"].double().view(8, 64, 1, 1), c["b"].double(), stride=2)
    assert float((nchw(c["pre"].want) - want).abs().max()) <= 1e-12 * float(c["pre"].abs_sum.max())
    for m in [(1, 33, 65), (2, 3, 5), (1, 1, 1)]:
        c = case_stem(m, "randn")
        conv = F.conv2d(nchw(c["img"]).double(), nchw(c["w"]).double(), c["b"].double(), stride=2, padding=3)
        want = F.max_pool2d(conv.relu(), 3, 2, 1)
        assert tuple(want.shape) == tuple(nchw(c["ref"].want).shape)
        assert float((nchw(c["ref"].want) - want).abs().max()) <= 1e-12 * float(c["ref"].abs_sum.max())
    lv = [torch.arange(6 * h * w * 2, dtype=F64).reshape(6, h, w, 2) + 1000 * j for j, (h, w) in enumerate(PYRAMID)]
    rows, written = R.token_rows(lv, 2, 3, sum(h * w for h, w in PYRAMID), [0, 44, 56, 59])
    want = torch.cat([v.reshape(2, 3, -1, 2) for v in lv], 2).flatten(1, 2)      # feature_maps_format's order, restated
    assert bool(written.all()) and torch.equal(rows, want)


def test_cancel_small_and_big_inputs_are_what_they_claim():
    for stride in (1, 2):
        c = case3((3, 9, 13), stride, (256, 192), "cancel")["pre"]
        inner = (slice(None), slice(1, -1), slice(1, -1))
        ratio = float((c.want[inner].abs() / c.abs_sum[inner]).median())
        print(f"FIG cancel 3x3 stride {stride}: median |want| / abs_sum = {ratio:.2e}")
        assert ratio < 3e-3
    c = case1((3, 9, 13), 1, 256, 192, "cancel", "res")["pre"]
    ratio = float((c.want.abs() / c.abs_sum).median())
    print(f"FIG cancel 1x1: median |want| / abs_sum = {ratio:.2e}")
    assert ratio < 1e-3
    c = case3((3, 9, 13), 1, (64, 72), "small")
    sub = 2.0 ** -14
    assert float((c["x"].float().abs() < sub).float().mean()) > 0.1 and float((c["pre"].want.abs() < sub).double().mean()) > 0.1
    c = case3((3, 9, 13), 1, (64, 72), "big")["pre"]
    assert float((c.want.abs() >= 2.0 ** 16 * 1.01).double().mean()) > 0.02
    w = coded_weights(192, 3, 3, 256)
    assert float(w.abs().max()) <= 1024 and bool((w[:, :, :, 1:] != w[:, :, :, :-1]).all()) and bool((w[1:] != w[:-1]).all())
    assert bool((w.reshape(192, 9, 256)[:, 1:] != w.reshape(192, 9, 256)[:, :-1]).all())
    assert torch.equal(h16(w).float(), w)


def test_tile_counts_reach_the_xcd_walk_edges():
    """gx * gy of the cases: 1, 7, 8, 9 and 17 on the direct (variants 1-4) and the staged (5-8) launch path."""
    for path in (range(1, 5), range(5, 9)):
        counts = set()
        for v in path:
            for m, stride, cp, _ in cases3(v):
                ho, wo = out_hw(m[1], m[2], stride)
                counts.add(tiles3(v, m[0] * ho * wo, cp[1]))
        print(f"FIG tile counts variants {list(path)}: {sorted(counts)}")
        assert {1, 7, 8, 9, 17} <= counts
    for m, cp, expect in SELECT3:
        assert chosen3(m[0] * m[1] * m[2], cp[1]) == expect
        assert chosen3((m[0] * m[1] - 1) * m[2], cp[1]) != expect          # one map row fewer: the choice in front of it


def test_fp32_reference_stays_under_half_of_the_bounds():
    """Two float32 references -- (i) torch's conv2d in float32, (ii) a float32 sum in the kernels' order -- with the operator's
    rounding points, on the operands of every GPU case of this module: the kappa each needs (conv_ref.kappa_needed) and its
    figure against (e). KAPPA is twice the largest kappa; both references stay under half of (e). Also: under 1 % of a `big`
    case lies in the unjudged overflow band."""
    worst, bands = {}, {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                # thousands of tiny products: a thread pool only waits on itself
    try:
        _fp32_references(worst, bands)
    finally:
        torch.set_num_threads(threads)
    top = max(worst.items(), key=lambda kv: kv[1][0])
    for (op, kind), (k, e, name) in sorted(worst.items()):
        print(f"FIG fp32 {op} {kind}: kappa needed {k:.3f} ({name}), figure against (e) {e:.3f}")
    print(f"FIG fp32 worst kappa {top[1][0]:.3f} by {top[0]} {top[1][2]}; KAPPA = {KAPPA} ({KAPPA_SET_BY})")
    for op, (band, total) in sorted(bands.items()):
        print(f"FIG big {op}: {band} of {total} elements in the unjudged overflow band = {band / total:.4f}")
        assert band < 0.01 * total, (op, band, total)
    assert 2 * top[1][0] <= KAPPA, (top, KAPPA)     # under half of the kappa term of (e)
    assert max(v[1] for v in worst.values()) <= 1.0


def _fp32_references(worst, bands):

    def note(op, kind, name, got, ref):
        if kind.startswith("onehot"):       # every sum is exact in fp32: nothing to measure
            assert bool((got.to(F64) == ref.want.to(torch.float16).to(F64)).all()), (op, name)
            return
        k, e = R.kappa_needed(got, ref), R.figure_e(got, ref, KAPPA, ref.want.abs() <= R.F16_MAX * 0.99)
        band = int(((ref.want.abs() < 2.0 ** 16 * 1.01) & (ref.want.abs() > R.F16_MAX * 0.99)).sum())
        if kind == "big":
            tot = bands.setdefault(op.split()[0], [0, 0])
            tot[0], tot[1] = tot[0] + band, tot[1] + ref.want.numel()
        else:
            assert band == 0, (op, name, "an output in the unjudged band")
        slot = worst.setdefault((op, kind[:6]), [0.0, 0.0, ""])
        if k >= slot[0]:
            slot[0], slot[2] = k, name
        slot[1] = max(slot[1], e)

    for key in sorted({k for v in range(9) for k in cases3(v)} | {((6,) + hw, 1, cp, kind) for hw in PYRAMID + [TOK_MAP[1:]]
                                                                   for cp in ((256, 256), (64, 72), (128, 64))
                                                                   for kind in ("randn", "onehot0", "onehot1")}):
        c = case3(*key)
        for order in ("torch", "taps"):
            v = R.conv3x3_pre32(c["x"], c["w"], c["b"], key[1], order)
            for relu in (False, True):
                note(f"conv3x3 {order}", key[3], str(key), R.finish_f32(v, relu), with_relu(c["pre"], relu))
    for cin in CIN1:
        for key in cases1(cin):
            c = case1(*key)
            for order in ("torch", "taps"):
                v = R.conv1x1_pre32(c["x"], c["w"], c["b"], c["res"], key[1], key[5] == "up", c["inb"], order)
                for relu in (False, True):
                    note(f"conv1x1 {order}", key[4], str(key), R.finish_f32(v, relu), with_relu(c["pre"], relu))
    for m in STEM_IMAGES:
        for kind in STEM_KINDS:
            c = case_stem(m, kind)
            for order in ("torch", "taps"):
                note(f"stem {order}", kind, str((m, kind)), R.stem_f32(c["img"], c["w"], c["b"], order), c["ref"])
    for c_ in EPI_C:
        for m in EPI_MAPS:
            for kind in EPI_KINDS:
                d = case_epi(m, c_, kind)
                note("bias_act", kind, str((m, c_, kind)), R.bias_act_f32(d["y"], d["b"], d["res"], False), R.bias_act(d["y"], d["b"], d["res"], False))
                note("bias_relu_maxpool", kind, str((m, c_, kind)), R.bias_relu_maxpool_f32(d["y"], d["b"]), R.bias_relu_maxpool(d["y"], d["b"]))
