"""Ungrouped attention (csrc/attention.hip, GROUPED = false) at key and query edges, against float64.

The kernels under test, each through plugin/ops.py or the C entry: attention_f32_kernel<false> (split=0),
attention_f16s_kernel<false> (split=1), attention_halfs_kernel<false, 8> (split=2: operands packed as the producing GEMM leaves
them, 1/8 folded into q; what every 3D self-attention, 900 x 900, and every temporal cross-attention, 900 x 600, of a frame
runs) and their three AltKeys instantiations behind simpb_attention_select. tests/test_attention_groups.py holds the GROUPED
half of the file; this module is its sibling and takes its bounds, its input kinds and its helpers from it.

Reference: _ref, plain float64 softmax(q k^T / 8) v per head and mag = P @ |v|. E = 512, 8 heads. Bounds (the project's own):
  (a) every output finite;
  (b) max |got - want| <= 2e-5 * max(1, max |want|);
  (c) per element |got - want| <= 2e-5 * (P @ |v|), not on the sharp_* inputs (plain fp32 torch misses it there);
  (d) split 1, 2: max error <= 4 x the split-0 kernel's on the same operands + 1e-7 * max (P @ |v|).
The CPU test test_fp32_formula_stays_under_half_of_each_bound holds the same formula in plain fp32 torch under HALF of every
bound that is asserted, for every case of the module. Bit-level statements are torch.equal on the output bits.
Measured figures of one MI355X run: profiles/attention_ungrouped_vs_float64.md.

Inputs: the eight kinds of the grouped module (randn, ramp_up / ramp_down with strength RAMP, sharp_* = the same three
times 4, grow / decay), seeded per (nq, nk, input). The ramp runs over the key slots. For grow / decay the key rows are times
0.1^j (decay) or 0.1^(jmax - j) (grow) with j = key // (keys per round of the kernel under test): 128 for splits 0 and 1, 256
for split 2 -- so splits 0 / 1 and split 2 get their own operands for these two kinds, and (d) compares split 2 with the exact
kernel on split 2's operands. Then a wave's running maximum never moves after its first tile (decay: alpha == 1 in every lane,
the eight-wave kernel's ballot(alpha != 1) is false and the rescale is skipped) or moves in every round (grow). The CPU test
test_decay_and_grow_move_the_running_maximum_as_described proves that in float64 for both layouts at nk = 900 and 1025.

Key-count sweep at nq = 65 (two full query tiles and one with a single live query), every split, every input. The path a
count reaches (tile = 32 keys; a round = one tile per wave):
  nk     four waves, 128 keys per round (split 0, 1)            eight waves, 256 keys per round (split 2)
  1, 31  wave 0 a partial tile, waves 1-3 own nothing           wave 0 alone, seven empty partners (both hand-over sides -inf)
  32     wave 0 one full tile, no masked key                    the same, the full-tile branch and nothing else
  33     wave 1 owns one key                                    wave 1 owns one key
  64     waves 0-1 full, waves 2-3 empty                        waves 0-1 full; waves 2-3 merge -inf with -inf
  127    partial tile on wave 3                                 partial tile on wave 3, waves 4-7 hand over nothing
  128    four full tiles: exactly one round, nothing masked     waves 0-3 full, every hand-over meets m = -inf
  129    wave 0's second round is one key                       wave 4 owns one key, waves 5-7 nothing
  160    that second tile is full                               wave 4 owns one full tile, waves 5-7 nothing
  161    wave 1's second round is one key                       wave 5 owns one key
  255    partial tile on wave 3, second round                   the partial tile is on wave 7
  256    two full rounds                                        eight full tiles, one round, no masked tile anywhere
  257    wave 0's third round is one key                        wave 0's second round is one key
  288    that tile is full                                      that second tile is full
  511    partial on wave 3, fourth round                        partial on wave 7, second round
  512    four full rounds                                       two full rounds
  513    one key in a fifth round                               one key in a third round
  600    shipped (temporal): 18 full tiles + 24 keys on wave 2  18 full tiles + 24 keys on wave 2, third round
  900    shipped (3D self): 28 full tiles + 4 keys on wave 0    28 full tiles + 4 keys on wave 4, fourth round
  1025   eight full rounds + one key in a ninth                 four full rounds + one key in a fifth
Query-count sweep: nq in {1, 31, 32, 33, 64, 65} at nk in {45, 257}, every split, every input."""
import ctypes
import math

import pytest
import torch

from tests.test_attention_groups import E, HEADS, INPUTS, RAMP, _ratios, _run
from tests.test_gpu_ops import _pack_split_halfs
from tests.test_gpu_stream_restart_ops import _poison

gpu = pytest.mark.gpu
SPLITS = [0, 1, 2]
NKS = [1, 31, 32, 33, 64, 127, 128, 129, 160, 161, 255, 256, 257, 288, 511, 512, 513, 600, 900, 1025]
NQS = [1, 31, 32, 33, 64, 65]
NQ_SWEEP_NKS = [45, 257]
NQ = 65
SELECT = (0, 1, 0)
SELECT_EDGES = [(256, 129), (1, 257)]
SENT = -777.25       # sentinel of the guarded output buffer
PAD = 4096           # floats on either side of it


# ---------------------------------------------------------------------------------------------------- inputs, reference
def _inputs(nq, nk, kind, period=128, bs=1):
    g = torch.Generator().manual_seed(((nq * 2048 + nk) * 16 + INPUTS.index(kind)) * 8 + bs)
    q = torch.randn(bs, nq, E, generator=g)
    k, v = torch.randn(bs, nk, E, generator=g), torch.randn(bs, nk, E, generator=g)
    base = kind[6:] if kind.startswith("sharp_") else kind
    if base in ("ramp_up", "ramp_down"):
        u = torch.randn(E, generator=g)
        r = torch.linspace(0, 1, nk) if base == "ramp_up" else torch.linspace(1, 0, nk)
        q = q + RAMP * u
        k = k + RAMP * r[None, :, None] * u
    elif base in ("grow", "decay"):
        j = torch.arange(nk) // period
        f = 0.1 ** ((j if base == "decay" else int(j[-1]) - j).float())
        k = k * f[None, :, None]
    if kind.startswith("sharp_"):
        q, k, v = q * 4, k * 4, v * 4
    return q, k, v


def _ref(q, k, v, dtype=torch.float64):
    """(want, mag): softmax(q k^T / 8) v per head and P @ |v|, evaluated in `dtype`."""
    bs, nq, _ = q.shape
    qh, kh, vh = (t.to(dtype).reshape(bs, t.shape[1], HEADS, 64).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(64), -1)
    return (p @ vh).transpose(1, 2).reshape(bs, nq, E), (p @ vh.abs()).transpose(1, 2).reshape(bs, nq, E)


_REF = {}


def _case(nq, nk, kind, period=128, bs=1):
    """Operands and their float64 reference, computed once; the cache holds the inputs of one (nq, nk, bs) at a time."""
    if kind not in ("grow", "decay"):
        period = 128
    key = (nq, nk, bs, kind, period)
    if key not in _REF:
        if any(o[:3] != key[:3] for o in _REF):
            _REF.clear()
        q, k, v = _inputs(nq, nk, kind, period, bs)
        _REF[key] = (q, k, v) + _ref(q, k, v)
    return _REF[key]


def _sweep_cases():
    """(input, keys per round it is made for, splits it is put to, whether (c) applies) of a sweep point: every input for
    every split; grow / decay once per round length, each for the splits whose kernel has that round."""
    for kind in INPUTS:
        with_c = not kind.startswith("sharp_")
        if kind in ("grow", "decay"):
            yield kind, 128, (0, 1), with_c
            yield kind, 256, (2,), with_c
        else:
            yield kind, 128, (0, 1, 2), with_c


def _select_operands(n1, n2):
    g = torch.Generator().manual_seed(4000 + 8 * n1 + n2)
    q = torch.randn(3, NQ, E, generator=g)
    return q, [(torch.randn(3, n, E, generator=g), torch.randn(3, n, E, generator=g)) for n in (n1, n2)]


def _chain_inputs(form):
    """x (as query | query_pos, two 256-wide segments), folded weights with 1/8 in the q rows (plugin/layers.py:183-196), and
    q, k, v in float64 from x. temporal: q from 900 rows, k | v from 600 other rows; self: q | k | v from the same 900 rows."""
    g = torch.Generator().manual_seed(81 if form == "temporal" else 82)
    nk = 600 if form == "temporal" else 900
    xq = torch.randn(1, 900, E, generator=g)
    xk = torch.randn(1, nk, E, generator=g) if form == "temporal" else xq
    w = torch.randn(3 * E, E, generator=g) / math.sqrt(E)
    bias = torch.randn(3 * E, generator=g) * 0.1
    rs = torch.cat([torch.full((E,), 0.125), torch.ones(2 * E)])
    w, bias = w * rs[:, None], bias * rs
    q = (xq.double() @ w[:E].double().t() + bias[:E].double()) * 8.0    # the unscaled q for the reference
    kv = xk.double() @ w[E:].double().t() + bias[E:].double()
    return xq, xk, w, bias, (q, kv[..., :E], kv[..., E:])


def _all_cases():
    """Every (operands, reference) pair a GPU test of this module holds against float64."""
    for nq, nk in [(NQ, nk) for nk in NKS] + [(nq, nk) for nk in NQ_SWEEP_NKS for nq in NQS if (nq, nk) != (NQ, 257)]:
        for kind, period, _, with_c in _sweep_cases():
            yield (nq, nk, "%s/%d" % (kind, period) if kind in ("grow", "decay") else kind), _case(nq, nk, kind, period), with_c
    yield (33, 45, "layout_bs2"), _case(33, 45, "randn", bs=2), True
    yield (NQ, 257, "odd_v"), _case(NQ, 257, "randn"), True
    for n1, n2 in SELECT_EDGES:
        q, sets = _select_operands(n1, n2)
        for b, s in enumerate(SELECT):
            ops = (q[b:b + 1], sets[s][0][b:b + 1], sets[s][1][b:b + 1])
            yield (NQ, (n1, n2)[s], "select%d_%d/stream%d" % (n1, n2, b)), ops + _ref(*ops), True
    for form in ("temporal", "self"):
        q, k, v = _chain_inputs(form)[4]
        yield (900, k.shape[1], "chain_" + form), (q.float(), k.float(), v.float()) + _ref(q, k, v), True


# ---------------------------------------------------------------------------------------------------- CPU
def test_fp32_formula_stays_under_half_of_each_bound():
    """The same formula in plain fp32 torch stays under HALF of every bound the GPU tests assert on that case: (b)
    everywhere, (c) on the non-sharp inputs. So a correct fp32-grade kernel can meet them."""
    over, worst = [], {}
    for what, (q, k, v, want, mag), with_c in _all_cases():
        got, _ = _ref(q, k, v, dtype=torch.float32)
        assert want.dtype == torch.float64 and got.dtype == torch.float32
        rb, rc = _ratios(got, want, mag)
        print("FP32|%d|%s|%s|b=%.3f|c=%.3f%s" % (what + (rb, rc, "" if with_c else "(n/a)")))
        for name, r in (("b", rb), ("c" if with_c else "c, not applied", rc)):
            if r > worst.get(name, (0.0,))[0]:
                worst[name] = (r, what)
        if rb > 0.5 or (with_c and rc > 0.5):
            over.append((what, rb, rc))
    print("FP32 worst:", worst)
    assert not over, over


def _tile_maxima(s, nk, waves, wave):
    """Per tile of `wave`: (maximum per (head, query), number of keys in the tile)."""
    return [(s[..., a:a + 32].amax(-1), min(32, nk - a)) for a in range(32 * wave, nk, 32 * waves)]


@pytest.mark.parametrize("nk", [900, 1025])
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("kind", ["decay", "grow"])
def test_decay_and_grow_move_the_running_maximum_as_described(kind, waves, nk):
    """In float64, per wave of the four-wave (decades 128 keys apart) and of the eight-wave layout (256 apart), on the two
    full query tiles of nq = 65: under decay no query's running maximum moves after the wave's first tile (every lane's
    alpha is exactly 1); under grow every query's moves in every later full tile, and in a later partial tile (4 keys at
    nk = 900, one key at 1025) the maximum of some query of every (head, query tile) moves, so the wave does rescale."""
    q, k, _, _, _ = _case(NQ, nk, kind, 32 * waves)
    s = (q[0, :64].double().reshape(64, HEADS, 64).transpose(0, 1) @ k[0].double().reshape(nk, HEADS, 64).permute(1, 2, 0)) / 8.0
    later, partial = 0, 0
    for wave in range(waves):
        tiles = _tile_maxima(s, nk, waves, wave)
        assert len(tiles) >= 3
        run = tiles[0][0]
        for t, keys in tiles[1:]:
            later += 1
            if kind == "decay":
                assert bool((t < run).all())
            elif keys == 32:
                assert bool((t > run).all())
            else:
                partial += 1
                assert bool((t > run).reshape(HEADS, 2, 32).any(-1).all())
            run = torch.maximum(run, t)
    assert later == (nk + 31) // 32 - waves and (kind == "decay" or partial == 1)


def _is_refused(a, entry):
    """The validation of csrc/attention.hip (check_args, with the second set's rules for the selector of
    simpb_attention_select) restated on the host: is call `a` turned away before any HIP call? The refusal test asserts this of every call BEFORE it makes it, so a
    case that is in fact a valid call fails the test on the host instead of launching on a placeholder address where a device
    is present. entry: "tables" (the three single-set entry points), "select_null" (no selector, takes no tables) or "select"."""
    e = a["heads"] * 64
    bad = not (a["out"] and a["q"] and a["k"] and a["v"]) or min(a["bs"], a["heads"], a["nq"], a["nk"]) <= 0
    bad = bad or a["hd"] != 64 or min(a["ldq"], a["ldk"], a["ldv"], a["ldo"]) < e
    bad = bad or (a["ldq"] | a["ldk"]) & 3 != 0 or (a["q"] | a["k"]) & 15 != 0
    bad = bad or a["bs"] > 65535 or a["heads"] > 65535
    if entry == "tables":
        bad = bad or (a["cam"] == 0) != (a["start"] == 0) or (a["cam"] != 0 and a["nk"] != a["nq"])
    if entry != "tables":
        bad = bad or not 0 <= a["split"] <= 2
    if entry == "select":
        bad = bad or not (a["k2"] and a["v2"]) or a["nk2"] <= 0 or min(a["ldk2"], a["ldv2"]) < e or a["ldk2"] & 3 != 0 or a["k2"] & 15 != 0
    return bool(bad)


def test_attention_entries_refuse_bad_arguments():
    """SIMPB_EINVAL in front of any HIP call, so no device is needed. Every call is the launch the GPU tests make (nq = 65,
    nk = 257; with tables nq = nk = 257) with exactly ONE defect, put to simpb_attention_f32, simpb_attention_f32_split and
    simpb_attention_split_halfs (splits 0, 1, 2); the cases without tables also to simpb_attention_select, without a selector
    and, splits 0, 1, 2, with one, where the second set obeys the rules of the first. Addresses are those of a host array,
    16-byte aligned; _is_refused guards every call."""
    from simpb_amd import _lib
    lib = _lib.lib()
    host = (ctypes.c_char * 8192)()
    A = (ctypes.addressof(host) + 63) // 64 * 64
    ok = dict(out=A, q=A, k=A, v=A, cam=0, start=0, bs=1, heads=HEADS, hd=64, nq=NQ, nk=257, ldq=E, ldk=E, ldv=E, ldo=E,
              k2=A, v2=A, select=A, nk2=129, ldk2=E, ldv2=E, split=0)
    with_tables = dict(ok, cam=A, start=A, nq=257)
    assert not _is_refused(ok, "tables") and not _is_refused(with_tables, "tables") and not _is_refused(ok, "select")   # one defect each
    wide = 65536 * 64
    plain = {
        "head_dim 32": dict(hd=32), "head_dim 128": dict(hd=128), "head_dim 65": dict(hd=65),
        "ldq under E": dict(ldq=E - 4), "ldk under E": dict(ldk=E - 4), "ldv under E": dict(ldv=E - 1), "ldo under E": dict(ldo=E - 1),
        "ldq % 4": dict(ldq=E + 2), "ldk % 4": dict(ldk=E + 1),
        "q off the 16-byte grid": dict(q=A + 4), "k off the 16-byte grid": dict(k=A + 8),
        "nk = 0": dict(nk=0), "nq = 0": dict(nq=0), "bs = 0": dict(bs=0),
        "bs 65536": dict(bs=65536), "heads 65536": dict(heads=65536, ldq=wide, ldk=wide, ldv=wide, ldo=wide, ldk2=wide, ldv2=wide),
        "null out": dict(out=0), "null q": dict(q=0), "null k": dict(k=0), "null v": dict(v=0),
    }
    tables = {
        "query_cam without group_start": dict(with_tables, start=0), "group_start without query_cam": dict(with_tables, cam=0),
        "tables with nq != nk": dict(with_tables, nq=NQ),
    }
    second = {
        "nk2 = 0": dict(nk2=0), "ldk2 under E": dict(ldk2=E - 4), "ldv2 under E": dict(ldv2=E - 1), "ldk2 % 4": dict(ldk2=E + 2),
        "k2 off the 16-byte grid": dict(k2=A + 4), "null k2": dict(k2=0), "null v2": dict(v2=0),
    }
    P = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    wrong = []

    def single(name, a):
        assert _is_refused(a, "tables"), (name, "would be a valid call")
        args = [P(a[n]) for n in ("out", "q", "k", "v", "cam", "start")] + [a[n] for n in ("bs", "heads", "hd", "nq", "nk", "ldq", "ldk", "ldv", "ldo")]
        for entry, status in (("f32", lib.simpb_attention_f32(*args, 0.125, None)), ("f32_split", lib.simpb_attention_f32_split(*args, 0.125, None)),
                              ("split_halfs", lib.simpb_attention_split_halfs(*args, None))):
            if status != 1:
                wrong.append((name, entry, status))

    def select(name, a, selector):
        assert _is_refused(a, "select" if selector else "select_null"), (name, "would be a valid call")
        status = lib.simpb_attention_select(a["split"], P(a["out"]), P(a["q"]), P(a["k"]), P(a["v"]), P(a["k2"]), P(a["v2"]),
                                            P(a["select"]) if selector else None, a["bs"], a["heads"], a["hd"], a["nq"], a["nk"], a["nk2"],
                                            a["ldq"], a["ldk"], a["ldv"], a["ldk2"], a["ldv2"], a["ldo"], 0.125, None)
        if status != 1:
            wrong.append((name, "select split %d%s" % (a["split"], "" if selector else ", no selector"), status))

    for name, change in plain.items():
        single(name, dict(ok, **change))
        for split in SPLITS:
            select(name, dict(ok, split=split, **change), False)
            select(name, dict(ok, split=split, **change), True)
    for name, a in tables.items():
        single(name, a)   # (simpb_attention_select takes no tables: these calls would be valid there)
    for name, change in second.items():
        for split in SPLITS:
            select(name, dict(ok, split=split, **change), True)
    for split in (3, -1):
        select("split %d" % split, dict(ok, split=split), True)
        select("split %d" % split, dict(ok, split=split), False)
    assert not wrong, wrong


# ---------------------------------------------------------------------------------------------------- GPU
def _check(got, exact, want, mag, with_c, what, fails):
    """(a)-(d) on one output; `exact` is the split-0 output on the same operands (None when `got` is that output). Prints the
    figures, appends what is over a bound to `fails` (the caller asserts after its last case)."""
    nq, nk, name, split = what
    rb, rc = _ratios(got, want, mag)
    err = float((got.double() - want).abs().max())
    rd = 0.0
    if exact is not None:
        e_exact = float((exact.double() - want).abs().max())
        rd = err / (4 * e_exact + 1e-7 * float(mag.max())) if err else 0.0
    print("RATIO|%d|%s|%s|split%d|b=%.3f|c=%.3f%s|d=%.3f" % (nq, nk, name, split, rb, rc, "" if with_c else "(n/a)", rd))
    if not bool(torch.isfinite(got).all()):
        fails.append((what, "(a) non-finite outputs", int((~torch.isfinite(got)).sum())))
    if not rb <= 1.0:
        fails.append((what, "(b) max error / (2e-5 * max(1, max |want|))", rb))
    if with_c and not rc <= 1.0:
        fails.append((what, "(c) error / (2e-5 * P @ |v|)", rc))
    if not rd <= 1.0:
        fails.append((what, "(d) max error / (4 x exact kernel's + 1e-7 max mag)", rd))


def _sweep_point(nq, nk, fails):
    for kind, period, splits, with_c in _sweep_cases():
        q, k, v, want, mag = _case(nq, nk, kind, period)
        exact = _run(q, k, v, 0)
        for split in splits:
            got = exact if split == 0 else _run(q, k, v, split)
            _check(got, None if split == 0 else exact, want, mag, with_c, (nq, nk, kind, split), fails)


@gpu
@pytest.mark.parametrize("nk", NKS)
def test_key_count_sweep_vs_float64(nk):
    """nq = 65, every input, every split: (a)-(d). See the module docstring for the path each count reaches."""
    fails = []
    _sweep_point(NQ, nk, fails)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("nk", NQ_SWEEP_NKS)
@pytest.mark.parametrize("nq", NQS)
def test_query_count_sweep_vs_float64(nq, nk):
    """One query, a tile short of one, a full tile, one over, two tiles, two and one: the q_ok lanes of the last tile."""
    fails = []
    _sweep_point(nq, nk, fails)
    assert not fails, fails


def _nan_rows(n, split):
    t = torch.empty(1, n, E)
    _poison(t, split)
    return t


def _as_launched(split, q, *kv):
    """CPU operands in the form the launch of that split reads (split 2: packed half pairs, 1/8 folded into q)."""
    if split == 2:
        return [_pack_split_halfs((q * 0.125).contiguous())] + [_pack_split_halfs(t.contiguous()) for t in kv]
    return [q] + list(kv)


def _launch(split, q, k, v):
    """attention_f32 on device operands that are already in the split's own form."""
    from simpb_amd.plugin.ops import attention_f32
    return attention_f32(q, k, v, HEADS, split=split)


@gpu
@pytest.mark.parametrize("split", SPLITS)
def test_two_launches_give_the_same_bits(split):
    for nk in (257, 600):
        q, k, v = (t.cuda() for t in _as_launched(split, *_case(NQ, nk, "randn")[:3]))
        first, second = _launch(split, q, k, v), _launch(split, q, k, v)
        assert bool(torch.isfinite(first).all()) and torch.equal(first, second), (split, nk)


@gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("nk", [33, 256, 600])
def test_rows_past_the_key_count_are_never_read(nk, split):
    """bs = 1, k and v the first nk rows of a buffer of nk + 40 rows whose other rows are NaN (split 2: both halfs): the bits of
    the launch on tight buffers. nk = 33: the clamped loads of a one-key tile; 256: the next-tile prefetch after full tiles
    only; 600: the shipped count."""
    q, k, v = _as_launched(split, *_case(NQ, nk, "randn")[:3])
    tight = _launch(split, q.cuda(), k.cuda(), v.cuda())
    kl, vl = (torch.cat([t, _nan_rows(40, split)], 1).cuda() for t in (k, v))
    for t in (kl, vl):   # the poison is in place, in the form the split reads
        assert bool(torch.isnan(t[:, nk:].view(torch.float16)).all()) if split == 2 else bool(torch.isnan(t[:, nk:]).all())
    loose = _launch(split, q.cuda(), kl[:, :nk], vl[:, :nk])
    assert bool(torch.isfinite(loose).all()), (split, nk, "NaN rows past the key count reached the output")
    assert torch.equal(tight, loose), (split, nk)


@gpu
@pytest.mark.parametrize("split", SPLITS)
def test_a_query_row_is_bitwise_independent_of_the_other_queries(split):
    """Queries 31, 32 and 33 (the last lane of one workgroup, the first two of the next) keep their bits when every other q
    row is replaced by fresh values times 64 (finite in half precision, also times 1/8)."""
    q, k, v, _, _ = _case(NQ, 257, "randn")
    g = torch.Generator().manual_seed(92)
    dirty_q = torch.randn(q.shape, generator=g) * 64
    dirty_q[:, 31:34] = q[:, 31:34]
    assert bool(torch.isfinite((dirty_q * 0.125).half()).all())
    clean = _run(q, k, v, split)
    dirty = _run(dirty_q, k, v, split)
    assert bool(torch.isfinite(dirty).all())
    others = [i for i in range(NQ) if i not in (31, 32, 33)]
    assert bool((clean[:, others] != dirty[:, others]).any(-1).all())   # the poison did reach every other row
    assert torch.equal(clean[:, 31:34], dirty[:, 31:34]), (split, int((clean[:, 31:34] != dirty[:, 31:34]).sum()))


@gpu
@pytest.mark.parametrize("split", SPLITS)
def test_a_query_row_gives_the_same_bits_at_every_slot(split):
    """One q row at slots 0, 31, 32 and 64 (first and last lane of a workgroup, first lane of the next, the only live lane of
    the last): the same 512 output values at each."""
    q, k, v, want, _ = _case(NQ, 257, "randn")
    q = q.clone()
    for s in (0, 31, 32, 64):
        q[:, s] = q[:, 7]
    got = _run(q, k, v, split)
    assert float((got[0, 7].double() - want[0, 7]).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))
    for s in (0, 31, 32, 64):
        assert torch.equal(got[0, s], got[0, 7]), (split, s, int((got[0, s] != got[0, 7]).sum()))


@gpu
@pytest.mark.parametrize("split", SPLITS)
def test_a_batch_row_is_bitwise_independent_of_the_other_batch_rows(split):
    """bs = 3: batch 1's rows are the bits of a bs = 1 launch on its operands, and keep them when batches 0 and 2 are replaced."""
    q, k, v, _, _ = _case(NQ, 257, "randn", bs=3)
    whole = _run(q, k, v, split)
    alone = _run(q[1:2], k[1:2], v[1:2], split)
    assert torch.equal(whole[1:2], alone), split
    g = torch.Generator().manual_seed(93)
    dirty = []
    for t in (q, k, v):
        p = torch.randn(t.shape, generator=g) * 64
        p[1] = t[1]
        dirty.append(p)
    again = _run(*dirty, split)
    assert bool(torch.isfinite(again).all())
    assert not torch.equal(again[0], whole[0]) and not torch.equal(again[2], whole[2])
    assert torch.equal(again[1], whole[1]), split


def _raw_launch(split, out_ptr, q, k_ptr, v_ptr, bs, nq, nk, ldq, ldk, ldv, ldo):
    """The C entry of a split on raw addresses (q a device tensor, the rest integers)."""
    from simpb_amd import _lib as L
    from simpb_amd.plugin.ops import _ptr, _stream
    lib = L.lib()
    args = [ctypes.c_void_p(out_ptr), _ptr(q), ctypes.c_void_p(k_ptr), ctypes.c_void_p(v_ptr), None, None, bs, HEADS, 64, nq, nk,
            ldq, ldk, ldv, ldo]
    if split == 2:
        status = lib.simpb_attention_split_halfs(*args, _stream())
    else:
        status = (lib.simpb_attention_f32_split if split else lib.simpb_attention_f32)(*args, 0.125, _stream())
    L.check(status, "attention split %d" % split)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("split", SPLITS)
def test_output_into_a_wider_buffer_writes_nothing_else(split):
    """bs = 2, nq = 33, ldo = E + 20 through the C entry: the [nq, E] blocks hold the bits of the launch with tight rows;
    the 20 pad columns of every row, three rows behind the last batch and 4096 floats on either side keep their sentinel."""
    bs, nq, nk, ldo, extra = 2, 33, 45, E + 20, 3
    q, k, v, want, mag = _case(nq, nk, "randn", bs=bs)
    qd, kd, vd = (t.cuda() for t in _as_launched(split, q, k, v))
    tight = _launch(split, qd, kd, vd)
    rows = bs * nq + extra
    whole = torch.full((2 * PAD + rows * ldo,), SENT, device="cuda")
    _raw_launch(split, whole.data_ptr() + 4 * PAD, qd, kd.data_ptr(), vd.data_ptr(), bs, nq, nk, E, E, E, ldo)
    body = whole[PAD:PAD + rows * ldo].view(rows, ldo)
    assert bool((whole[:PAD] == SENT).all()) and bool((whole[PAD + rows * ldo:] == SENT).all()), "write outside the buffer"
    assert bool((body[:, E:] == SENT).all()), "write into the pad columns"
    assert bool((body[bs * nq:] == SENT).all()), "write into rows past the last query"
    got = body[:bs * nq, :E].reshape(bs, nq, E)
    assert torch.equal(got, tight), split
    fails = []
    _check(got.cpu(), None, want, mag, True, (nq, nk, "layout_bs2", split), fails)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("split", SPLITS)
def test_v_at_an_odd_offset_with_an_odd_stride_vs_float64(split):
    """include/simpb_hip.h asks 16-byte alignment and a stride multiple of four of q and k only, and the kernels read v one
    float at a time: v one float into its allocation with ldv = E + 3 is a legal call. Held here as accepted and right; the
    three floats between rows are NaN (split 2: NaN half pairs)."""
    nq, nk, ldv = NQ, 257, E + 3
    q, k, v, want, mag = _case(nq, nk, "randn")
    qd, kd, vt = _as_launched(split, q, k, v)
    flat = torch.empty(1 + nk * ldv + 64)
    _poison(flat, split)
    torch.as_strided(flat, (nk, E), (ldv, 1), 1).copy_(vt[0])
    flat, qd, kd = flat.cuda(), qd.cuda(), kd.cuda()
    assert (flat.data_ptr() + 4) % 8 == 4 and ldv % 2 == 1
    out = torch.full((1, nq, E), SENT, device="cuda")
    _raw_launch(split, out.data_ptr(), qd, kd.data_ptr(), flat.data_ptr() + 4, 1, nq, nk, E, E, ldv, E)
    exact = out
    if split:
        exact = torch.full((1, nq, E), SENT, device="cuda")
        flat0 = torch.full((1 + nk * ldv + 64,), float("nan"))
        torch.as_strided(flat0, (nk, E), (ldv, 1), 1).copy_(v[0])
        flat0 = flat0.cuda()
        _raw_launch(0, exact.data_ptr(), q.cuda(), k.cuda().data_ptr(), flat0.data_ptr() + 4, 1, nq, nk, E, E, ldv, E)
    fails = []
    _check(out.cpu(), exact.cpu() if split else None, want, mag, True, (nq, nk, "odd_v", split), fails)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("form", ["temporal", "self"])
def test_shipped_chain_at_shipped_size_vs_float64(form):
    """What plugin/layers.py launches, against float64 computed from x. temporal: dense.gemm of two jobs with split_halfs
    output (q from 900 rows, k | v from 600 cached rows) into the eight-wave kernel; self: dense.linear q | k | v with
    split_halfs, 900 x 900."""
    from simpb_amd.plugin import dense
    xq, xk, w, bias, (q, k, v) = _chain_inputs(form)
    want, mag = _ref(q, k, v)
    wd, bd = w.cuda(), bias.cuda()
    seg = lambda x: [x[..., :256].contiguous().cuda(), x[..., 256:].contiguous().cuda()]   # noqa: E731  (query | query_pos)
    if form == "temporal":
        qp, kv = dense.gemm(dense.job(seg(xq), wd[:E], bd[:E], split_halfs=True), dense.job(seg(xk), wd[E:], bd[E:], split_halfs=True))
        kp, vp = kv[..., :E], kv[..., E:]
    else:
        qkv = dense.linear(seg(xq), wd, bd, split_halfs=True)
        qp, kp, vp = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    assert kp.stride(1) in (2 * E, 3 * E)
    got = _launch(2, qp, kp, vp).cpu()
    exact = _run(q.float(), k.float(), v.float(), 0)
    fails = []
    _check(got, exact, want, mag, True, (900, k.shape[1], "chain_" + form, 2), fails)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("n1,n2", SELECT_EDGES)
def test_select_at_key_count_edges(n1, n2, split):
    """attention_select, bs = 3, select (0, 1, 0), nq = 65. (256, 129): streams 0 and 2 take the no-masked-tile path, stream 1
    a one-key tile; (1, 257): one key against a second round of one key. Each stream is bit-equal to the ungrouped launch
    on its own set -- so the chosen Nk reached the full-tile test and the round count -- and within (b) of float64."""
    from simpb_amd.plugin.ops import attention_select
    q, sets = _select_operands(n1, n2)
    qd, k1, v1, k2, v2 = (t.cuda() for t in _as_launched(split, q, sets[0][0], sets[0][1], sets[1][0], sets[1][1]))
    got = attention_select(qd, k1, v1, k2, v2, torch.tensor(SELECT, dtype=torch.uint8, device="cuda"), HEADS, split=split)
    fails = []
    for b, s in enumerate(SELECT):
        kd, vd = (k2, v2) if s else (k1, v1)
        alone = _launch(split, qd[b:b + 1], kd[b:b + 1], vd[b:b + 1])
        if not torch.equal(got[b:b + 1], alone):
            fails.append((b, "not the bits of the launch on the selected set", int((got[b:b + 1] != alone).sum())))
        ops = (q[b:b + 1], sets[s][0][b:b + 1], sets[s][1][b:b + 1])
        want, mag = _ref(*ops)
        rb, rc = _ratios(got[b:b + 1].cpu(), want, mag)
        print("RATIO|%d|%d|select%d_%d/stream%d|split%d|b=%.3f|c=%.3f|d=0.000" % (NQ, (n1, n2)[s], n1, n2, b, split, rb, rc))
        if not (bool(torch.isfinite(got[b]).all()) and rb <= 1.0):
            fails.append((b, "(b)", rb))
    assert not fails, fails
