"""GPU: the entry points a per-stream restart adds (csrc/attention.hip simpb_attention_select, csrc/bank.hip
simpb_bank_get_restart / simpb_bank_cache_streams_restart) through ctypes and plugin/ops.py.

Attention: per batch row the comparator is TODAY'S entry point on the operands the row selected (bit for bit) and float64
(bound (b) of tests/test_attention_groups.py). Bank: the old entry points for the streams that go on (bit for bit) and the
PyTorch statement of InstanceBank.cache / get_instance_id, applied per stream with confidence=None for the restarted one."""
import ctypes

import pytest
import torch

from tests.test_gpu_ops import _pack_split_halfs

pytestmark = pytest.mark.gpu

HEADS, E, BS, NQ = 8, 512, 3, 100   # 100 queries: four query tiles, the last one partial
SELECT = (0, 1, 0)


def _lib():
    from simpb_amd import _lib as L
    from simpb_amd.plugin.ops import _ptr, _stream
    return L, L.lib(), _ptr, _stream


def _u8(flags):
    return torch.tensor(flags, dtype=torch.uint8, device="cuda")


# ----------------------------------------------------------------------------------------------------------------- attention
def _operands(n1, n2, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(BS, NQ, E, generator=g)
    k1, v1 = torch.randn(BS, n1, E, generator=g), torch.randn(BS, n1, E, generator=g)
    k2, v2 = torch.randn(BS, n2, E, generator=g), torch.randn(BS, n2, E, generator=g)
    return q, k1, v1, k2, v2


def _device(split, q, *kv):
    """Operands as the launch of that split takes them (split 2: packed half pairs, 1/8 folded into q)."""
    if split == 2:
        return [_pack_split_halfs((q * 0.125).contiguous()).cuda()] + [_pack_split_halfs(t.contiguous()).cuda() for t in kv]
    return [q.cuda()] + [t.cuda() for t in kv]


def _poison(t, split):
    """Every word a NaN (split 2: both halfs of the packed word)."""
    if split == 2:
        t.view(torch.int32).fill_(0x7E007E00)
    else:
        t.fill_(float("nan"))


def _want64(q, k, v):
    qh, kh, vh = (t.double().reshape(t.shape[0], t.shape[1], HEADS, 64).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) / 8.0, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(q.shape[0], q.shape[1], E)


@pytest.mark.parametrize("split", [0, 1, 2])
@pytest.mark.parametrize("n1,n2", [(600, 900), (24, 68)], ids=["shipped", "short_tiles"])
def test_attention_with_a_selector_is_todays_launch_on_the_selected_set(n1, n2, split):
    """bs 3, select (0, 1, 0). (600, 900): the shipped pair, neither a multiple of the 32-key tile; (24, 68): one short tile
    / two tiles plus four keys. Row by row bit-equal to attention_f32 on the selected operands; within 2e-5 * max(1, max
    |want|) of float64; and with every UNSELECTED set filled with NaN the output is the clean run's, bit for bit."""
    from simpb_amd.plugin.ops import attention_f32, attention_select
    ops = _operands(n1, n2, 7 + n1 + split)
    q, k1, v1, k2, v2 = _device(split, *ops)
    sel = _u8(SELECT)
    got = attention_select(q, k1, v1, k2, v2, sel, HEADS, split=split)
    for b, s in enumerate(SELECT):
        k, v = (k2, v2) if s else (k1, v1)
        alone = attention_f32(q[b:b + 1], k[b:b + 1], v[b:b + 1], HEADS, split=split)
        assert torch.equal(got[b:b + 1], alone), (b, "not the bits of the launch on the selected set")
        kk, vv = (ops[3], ops[4]) if s else (ops[1], ops[2])
        want = _want64(ops[0][b:b + 1], kk[b:b + 1], vv[b:b + 1])
        err = float((got[b:b + 1].cpu().double() - want).abs().max())
        bound = 2e-5 * max(1.0, float(want.abs().max()))
        print("select split%d n=(%d,%d) row %d: err %.3e bound %.3e" % (split, n1, n2, b, err, bound))
        assert err <= bound, (b, err, bound)
    for b, s in enumerate(SELECT):   # poison what row b did not select
        for t in ((k1, v1) if s else (k2, v2)):
            _poison(t[b], split)
    torch.cuda.synchronize()
    again = attention_select(q, k1, v1, k2, v2, sel, HEADS, split=split)
    assert bool(torch.isfinite(again).all()) and torch.equal(again, got)
    # a null selector: every row reads set 1 through today's kernel (row 1's set 1 is poisoned now: use rows 0 and 2)
    L, lib, P, S = _lib()
    out = torch.empty_like(got)
    L.check(lib.simpb_attention_select(split, P(out), P(q), P(k1), P(v1), None, None, None, BS, HEADS, 64, NQ, n1, n2, E, E, E, E, E,
                                       E, 0.125, S()), "simpb_attention_select")
    assert torch.equal(out[0], got[0]) and torch.equal(out[2], got[2])


def test_attention_select_takes_strided_views_of_projection_buffers():
    """What the head passes: k | v as column ranges of one [bs, N, 2E] buffer each, different row strides per set."""
    from simpb_amd.plugin.ops import attention_f32, attention_select
    g = torch.Generator().manual_seed(3)
    q = torch.randn(BS, NQ, E, generator=g).cuda()
    kv1, kv2 = torch.randn(BS, 40, 2 * E, generator=g).cuda(), torch.randn(BS, 70, 3 * E, generator=g).cuda()
    got = attention_select(q, kv1[..., :E], kv1[..., E:], kv2[..., E:2 * E], kv2[..., 2 * E:], _u8((1, 0, 1)), HEADS, split=0)
    for b, s in enumerate((1, 0, 1)):
        k, v = (kv2[..., E:2 * E], kv2[..., 2 * E:]) if s else (kv1[..., :E], kv1[..., E:])
        assert torch.equal(got[b:b + 1], attention_f32(q[b:b + 1], k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), HEADS, split=0))


def test_attention_select_refuses_bad_arguments():
    """EINVAL before any launch: a selector without a second set, a misaligned second key pointer, a row stride that is
    short or no multiple of four floats, an unknown split."""
    _, lib, _, _ = _lib()
    p = lambda a: ctypes.c_void_p(a)   # noqa: E731  (never dereferenced: validation comes first)
    ok = dict(split=0, out=p(4096), q=p(4096), k=p(4096), v=p(4096), k2=p(4096), v2=p(4096), select=p(64), ldk2=E, ldv2=E)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.simpb_attention_select(a["split"], a["out"], a["q"], a["k"], a["v"], a["k2"], a["v2"], a["select"], BS, HEADS, 64, NQ,
                                          24, 68, E, E, E, a["ldk2"], a["ldv2"], E, 0.125, None)

    assert call(k2=None) == 1 and call(v2=None) == 1 and call(k2=None, v2=None) == 1
    assert call(k2=p(4096 + 8)) == 1                       # 16-byte alignment of the key rows
    assert call(ldk2=E - 4) == 1 and call(ldv2=E - 1) == 1  # short
    assert call(ldk2=E + 2) == 1                           # not a multiple of four floats
    assert call(split=3) == 1 and call(split=-1) == 1


# ---------------------------------------------------------------------------------------------------------------------- bank
A, T, C, EMB = 48, 32, 10, 16
DECAY = 0.6


def test_bank_get_restart_masks_the_stream_out_and_leaves_the_others_as_they_were():
    L, lib, P, S = _lib()
    g = torch.Generator().manual_seed(1)
    anchor = torch.randn(BS, T, 11, generator=g)
    anchor[1] = float("nan")    # what the restarted slot held
    anchor = anchor.cuda()
    mats = torch.eye(4).repeat(BS, 1, 1) + 0.01 * torch.randn(BS, 4, 4, generator=g)
    mats, dt = mats.cuda(), torch.tensor([0.5, 0.0, 1.5]).cuda()   # (the runner stages dt = 0 for a restarted stream)

    def get(restart, use_new):
        out = torch.empty(BS, T, 11, device="cuda")
        mask, ti = torch.full((BS,), 7, dtype=torch.uint8, device="cuda"), torch.empty(BS, device="cuda")
        if use_new:
            L.check(lib.simpb_bank_get_restart(P(out), P(mask), P(ti), P(anchor), P(mats), P(dt), BS, T, 2.0, 0.25,
                                               P(restart) if restart is not None else None, S()), "bank_get_restart")
        else:
            L.check(lib.simpb_bank_get(P(out), P(mask), P(ti), P(anchor), P(mats), P(dt), BS, T, 2.0, 0.25, S()), "bank_get")
        torch.cuda.synchronize()
        return out, mask, ti

    old = get(None, False)
    null = get(None, True)
    new = get(_u8((0, 1, 0)), True)
    assert old[1].tolist() == [1, 1, 1] and old[2].tolist() == [0.5, 0.25, 1.5]
    for a, b in zip(old, null):   # NULL flags: the old entry point (bytes: row 1 is NaN)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert new[1].tolist() == [1, 0, 1] and new[2].tolist() == [0.5, 0.25, 1.5]
    for b in (0, 2):
        assert torch.equal(new[0][b], old[0][b])
    # a restart wins over a usable time step as well
    dt.copy_(torch.tensor([0.5, 0.75, 1.5]))
    m = get(_u8((0, 1, 1)), True)
    assert m[1].tolist() == [1, 0, 0] and m[2].tolist() == [0.5, 0.25, 0.25]


def _state(g, bs):
    iid = torch.randint(0, 500, (bs, A), generator=g)
    iid[torch.rand(bs, A, generator=g) < 0.5] = -1
    iid[:, T:] = -1   # (as update_instance_id leaves it)
    return dict(conf=torch.rand(bs, T, generator=g).cuda(), cf=torch.randn(bs, T, EMB, generator=g).cuda(),
                ca=torch.randn(bs, T, 11, generator=g).cuda(), iid=iid.cuda(), prev=torch.tensor(1234).cuda())


def _frame(g, bs):
    return (torch.randn(bs, A, EMB, generator=g).cuda(), torch.randn(bs, A, 11, generator=g).cuda(),
            (torch.randn(bs, A, C, generator=g) * 2).cuda())


def _commit(st, inputs, bs, thr, sync, restart=None, hold=None, old_entry=False):
    L, lib, P, S = _lib()
    feat, anchor, cls = inputs
    ids_out = torch.full((bs, A), -7, dtype=torch.long, device="cuda")
    scratch = torch.zeros(bs, T, dtype=torch.int32, device="cuda")
    args = [P(st["conf"]), P(st["cf"]), P(st["ca"]), P(st["iid"]), P(st["prev"]), P(ids_out), P(scratch), P(feat), P(anchor), P(cls),
            bs, A, C, T, EMB, 1, DECAY, 0 if thr is None else 1, 0.0 if thr is None else thr,
            P(hold) if hold is not None else None, 0 if hold is None else hold.numel(), None, P(sync) if sync is not None else None]
    if old_entry:
        L.check(lib.simpb_bank_cache_streams(*args, S()), "bank_cache_streams")
    else:
        L.check(lib.simpb_bank_cache_streams_restart(*args, None, P(restart) if restart is not None else None, S()),
                "bank_cache_streams_restart")
    torch.cuda.synchronize()
    return ids_out


def _statement(st, inputs, flags, thr):
    """InstanceBank.cache + get_instance_id + update_instance_id in PyTorch on the host, stream by stream, with
    confidence=None for a restarted stream whose ids the merge has reset (instance_bank.py:152-196). Returns the state
    the commit leaves and the ids it hands out."""
    feat, anchor, cls = (t.cpu() for t in inputs)
    out = {k: v.cpu().clone() for k, v in st.items()}
    ids_all, next_id = [], int(out["prev"])
    for b, cold in enumerate(flags):
        fresh_score = cls[b].max(dim=-1).values.sigmoid()
        score = fresh_score.clone()
        if not cold:
            score[:T] = torch.maximum(out["conf"][b] * DECAY, score[:T])
        order = torch.sort(score, descending=True, stable=True).indices[:T]
        ids = out["iid"][b].clone()
        fresh = ids < 0
        if thr is not None:
            fresh &= fresh_score >= thr
        ids[fresh] = next_id + torch.arange(int(fresh.sum()))
        next_id += int(fresh.sum())
        out["conf"][b], out["cf"][b], out["ca"][b] = score[order], feat[b][order], anchor[b][order]
        out["iid"][b] = torch.cat([ids[order], torch.full((A - T,), -1, dtype=torch.long)])
        ids_all.append(ids)
    out["prev"] = torch.tensor(next_id)
    return out, torch.stack(ids_all)


@pytest.mark.parametrize("thr", [None, 0.3], ids=["no_threshold", "threshold"])
@pytest.mark.parametrize("form", ["serial_bs1", "serial_bs3", "per_stream_bs3"])
def test_bank_commit_with_a_restarted_stream(form, thr):
    """Both commit kernels: the serial one at bs 1 (restarted) and bs 3, the per-stream one at bs 3, flags (0, 1, 0). The
    restarted stream's old confidence / feature / anchor rows hold NaN and its ids are -1 (what the merge leaves): the
    commit equals the PyTorch statement with confidence=None for it, no NaN survives, and the other streams' rows are bit
    for bit what the old entry point commits without any flag (their fresh ids up to the shift by the ids the restarted
    stream takes in front of them)."""
    bs = 1 if form == "serial_bs1" else BS
    flags = (1,) if bs == 1 else (0, 1, 0)
    g = torch.Generator().manual_seed(21 + bs)
    st = _state(g, bs)
    for b, cold in enumerate(flags):
        if cold:
            st["conf"][b], st["cf"][b], st["ca"][b], st["iid"][b] = float("nan"), float("nan"), float("nan"), -1
    inputs = _frame(g, bs)
    want, want_ids = _statement(st, inputs, flags, thr)
    plain = {k: v.clone() for k, v in st.items()}
    for b, cold in enumerate(flags):   # the comparator without a flag needs finite rows to rank
        if cold:
            plain["conf"][b] = 0.0
    sync = torch.zeros(2, dtype=torch.int32, device="cuda") if form == "per_stream_bs3" else None
    sync_p = torch.zeros(2, dtype=torch.int32, device="cuda") if form == "per_stream_bs3" else None
    ids = _commit(st, inputs, bs, thr, sync, restart=_u8(flags))
    ids_plain = _commit(plain, inputs, bs, thr, sync_p, old_entry=True)
    for k in ("conf", "cf", "ca", "iid"):
        assert not torch.isnan(st[k].float()).any(), k
    assert torch.equal(ids.cpu(), want_ids) and int(st["prev"]) == int(want["prev"]) > 1234
    assert torch.equal(st["iid"].cpu(), want["iid"]) and torch.equal(st["cf"].cpu(), want["cf"]) and torch.equal(st["ca"].cpu(), want["ca"])
    assert float((st["conf"].cpu() - want["conf"]).abs().max()) <= 1e-6   # (sigmoid: expf on the device, exp on the host)
    for b, cold in enumerate(flags):
        if cold:
            continue
        for k in ("conf", "cf", "ca"):
            assert torch.equal(st[k][b], plain[k][b]), (k, b)
        # ids: the same instances are fresh in both, numbered from a different start
        a, p = st["iid"][b], plain["iid"][b]
        assert torch.equal(a < 0, p < 0) and torch.equal(ids[b] < 0, ids_plain[b] < 0)
        kept = (a >= 0) & (a < 1234)
        assert torch.equal(a[kept], p[kept]) and torch.equal((a >= 1234), (p >= 1234))
    if sync is not None:
        assert sync.tolist() == [BS, 1]


@pytest.mark.parametrize("per_stream", [False, True], ids=["serial", "sync_words"])
def test_bank_commit_with_null_flags_is_the_old_entry_point(per_stream):
    g = torch.Generator().manual_seed(6)
    a = _state(g, BS)
    b = {k: v.clone() for k, v in a.items()}
    inputs = _frame(g, BS)
    sa, sb = ((torch.zeros(2, dtype=torch.int32, device="cuda") if per_stream else None) for _ in range(2))
    ia = _commit(a, inputs, BS, 0.3, sa, old_entry=True)
    ib = _commit(b, inputs, BS, 0.3, sb, restart=None)
    assert torch.equal(ia, ib) and all(torch.equal(a[k], b[k]) for k in a)
    ic = _commit(b, inputs, BS, 0.3, sb, restart=_u8((0, 0, 0)))   # all zero: the same again, on the state the first left
    id_ = _commit(a, inputs, BS, 0.3, sa, old_entry=True)
    assert torch.equal(ic, id_) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("per_stream", [False, True], ids=["serial", "sync_words"])
def test_bank_commit_with_a_hold_flag_leaves_a_restarted_stream_as_found(per_stream):
    g = torch.Generator().manual_seed(5)
    st = _state(g, BS)
    st["conf"][1] = float("nan")
    before = {k: v.clone() for k, v in st.items()}
    sync = torch.zeros(2, dtype=torch.int32, device="cuda") if per_stream else None
    hold = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    ids = _commit(st, _frame(g, BS), BS, None, sync, restart=_u8((0, 1, 0)), hold=hold)
    for k in st:
        assert torch.equal(st[k].reshape(-1).view(torch.uint8), before[k].reshape(-1).view(torch.uint8)), k
    assert bool((ids == -7).all())
    if per_stream:
        assert sync.tolist() == [0, 0]
