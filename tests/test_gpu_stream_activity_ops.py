"""GPU: the three `_active` entry points (csrc/alloc.hip, csrc/bank.hip) through ctypes. The comparator is always the
EXISTING entry point on the compacted sub-batch of active streams: the kernels treat streams independently apart from the
numbering of fresh track ids, which the sub-batch reproduces exactly, so every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from simpb_amd import synth

pytestmark = pytest.mark.gpu

BS, A, T, E, C = 3, 48, 32, 16, 10


def _lib():
    from simpb_amd import _lib as L
    from simpb_amd.plugin.ops import _ptr, _stream
    return L, L.lib(), _ptr, _stream


def _u8(mask):
    return torch.tensor(mask, dtype=torch.uint8, device="cuda")


# --------------------------------------------------------------------------------------------------------------- bank commit
def _bank_state(g):
    iid = torch.randint(0, 500, (BS, A), generator=g)
    iid[torch.rand(BS, A, generator=g) < 0.5] = -1   # some tracked, some waiting for an id
    return dict(conf=torch.rand(BS, T, generator=g).cuda(), cf=torch.randn(BS, T, E, generator=g).cuda(),
                ca=torch.randn(BS, T, 11, generator=g).cuda(), iid=iid.cuda(), prev=torch.tensor(1234).cuda())


def _frame_inputs(g, mask):
    feat, anchor = torch.randn(BS, A, E, generator=g), torch.randn(BS, A, 11, generator=g)
    cls = torch.randn(BS, A, C, generator=g) * 2
    for b, a in enumerate(mask):
        if not a:   # what a paused stream's rows hold must never be read
            feat[b], anchor[b], cls[b] = float("nan"), float("nan"), float("nan")
    return feat.cuda(), anchor.cuda(), cls.cuda()


def _commit(st, inputs, bs, thr, sync, active=None, hold=None, fill=-7):
    L, lib, P, S = _lib()
    feat, anchor, cls = inputs
    ids_out = torch.full((bs, A), fill, dtype=torch.long, device="cuda")
    scratch = torch.zeros(bs, T, dtype=torch.int32, device="cuda")
    args = [P(st["conf"]), P(st["cf"]), P(st["ca"]), P(st["iid"]), P(st["prev"]), P(ids_out), P(scratch), P(feat), P(anchor), P(cls),
            bs, A, C, T, E, 1, 0.6, 0 if thr is None else 1, 0.0 if thr is None else thr,
            P(hold) if hold is not None else None, 0 if hold is None else hold.numel(), None, P(sync) if sync is not None else None]
    if active is None:
        L.check(lib.simpb_bank_cache_streams(*args, S()), "bank_cache_streams")
    else:
        L.check(lib.simpb_bank_cache_streams_active(*args, P(active), S()), "bank_cache_streams_active")
    return ids_out


@pytest.mark.parametrize("thr", [None, 0.3], ids=["no_threshold", "threshold"])
@pytest.mark.parametrize("per_stream", [False, True], ids=["serial", "sync_words"])
@pytest.mark.parametrize("mask", [(1, 0, 1), (0, 1, 1), (1, 1, 0), (1, 1, 1)], ids=lambda m: "".join(map(str, m)))
def test_bank_commit_with_paused_streams_equals_the_commit_of_the_active_sub_batch(mask, per_stream, thr):
    """Two commits back to back (no host wait between them; with sync words that is two epochs of the meeting, with the
    paused stream's workgroup arriving in both). (0,1,1): the count "fresh instances in front of me" skips a paused stream;
    (1,1,0): the last workgroup writes prev_id although it is paused."""
    g = torch.Generator().manual_seed(11 + sum(m << i for i, m in enumerate(mask)))
    act = [b for b, a in enumerate(mask) if a]
    full = _bank_state(g)
    before = {k: v.clone() for k, v in full.items()}
    sub = {k: (v[act].clone() if v.dim() else v.clone()) for k, v in full.items()}
    sync_f = torch.zeros(2, dtype=torch.int32, device="cuda") if per_stream else None
    sync_s = torch.zeros(2, dtype=torch.int32, device="cuda") if per_stream else None
    active = _u8(mask)
    frames = [_frame_inputs(g, mask) for _ in range(2)]
    ids_f = [_commit(full, fr, BS, thr, sync_f, active=active) for fr in frames]
    ids_s = [_commit(sub, tuple(x[act].contiguous() for x in fr), len(act), thr, sync_s) for fr in frames]
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(ids_f[k][act], ids_s[k]), k
        for b, a in enumerate(mask):
            if not a:
                assert bool((ids_f[k][b] == -1).all())
    for name in ("conf", "cf", "ca", "iid"):
        assert torch.equal(full[name][act], sub[name]), name
        for b, a in enumerate(mask):
            if not a:   # (bytes: a NaN would compare unequal to itself)
                assert torch.equal(full[name][b].view(torch.uint8), before[name][b].view(torch.uint8)), (name, b)
        assert not torch.isnan(full[name].float()).any()
    assert int(full["prev"]) == int(sub["prev"]) > 1234
    if per_stream:   # every workgroup of the full batch arrived, twice
        assert sync_f.tolist() == [2 * BS, 2] and sync_s.tolist() == [2 * len(act), 2]


@pytest.mark.parametrize("per_stream", [False, True], ids=["serial", "sync_words"])
def test_bank_commit_with_a_hold_flag_writes_nothing_for_anyone(per_stream):
    g = torch.Generator().manual_seed(5)
    st = _bank_state(g)
    before = {k: v.clone() for k, v in st.items()}
    sync = torch.zeros(2, dtype=torch.int32, device="cuda") if per_stream else None
    hold = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    ids = _commit(st, _frame_inputs(g, (1, 0, 1)), BS, None, sync, active=_u8((1, 0, 1)), hold=hold)
    torch.cuda.synchronize()
    for k in st:
        assert torch.equal(st[k], before[k]), k
    assert bool((ids == -7).all())
    if per_stream:
        assert sync.tolist() == [0, 0]


def test_null_mask_equals_the_entry_point_without_one():
    L, lib, P, S = _lib()
    g = torch.Generator().manual_seed(6)
    a, b = _bank_state(g), None
    b = {k: v.clone() for k, v in a.items()}
    inputs = _frame_inputs(g, (1, 1, 1))
    sa, sb = (torch.zeros(2, dtype=torch.int32, device="cuda") for _ in range(2))
    ia = _commit(a, inputs, BS, 0.3, sa)
    feat, anchor, cls = inputs
    ib = torch.full((BS, A), -7, dtype=torch.long, device="cuda")
    scratch = torch.zeros(BS, T, dtype=torch.int32, device="cuda")
    L.check(lib.simpb_bank_cache_streams_active(
        P(b["conf"]), P(b["cf"]), P(b["ca"]), P(b["iid"]), P(b["prev"]), P(ib), P(scratch), P(feat), P(anchor), P(cls), BS, A, C, T, E,
        1, 0.6, 1, 0.3, None, 0, None, P(sb), None, S()), "bank_cache_streams_active")
    torch.cuda.synchronize()
    assert torch.equal(ia, ib) and all(torch.equal(a[k], b[k]) for k in a) and sa.tolist() == sb.tolist() == [BS, 1]


# --------------------------------------------------------------------------------------------------------------------- merge
def _merge(iid, cur_f, cur_a, cached_f, cached_a, index, mask, bs, active=None):
    L, lib, P, S = _lib()
    out_f, out_a = torch.empty(bs, A, E, device="cuda"), torch.empty(bs, A, 11, device="cuda")
    args = [P(out_f), P(out_a), None, P(iid), P(index), P(cur_f), P(cur_a), None, P(cached_f), P(cached_a), None, P(mask), None, 0,
            None, bs, A, T, E, 0]
    if active is None:
        L.check(lib.simpb_bank_update_merge(*args, S()), "bank_update_merge")
    else:
        L.check(lib.simpb_bank_update_merge_active(*args, P(active), S()), "bank_update_merge_active")
    return out_f, out_a


def test_merge_keeps_the_track_ids_of_a_paused_stream_that_is_masked_out():
    g = torch.Generator().manual_seed(3)
    iid = torch.randint(0, 500, (BS, A), generator=g).cuda()
    cur_f, cur_a = torch.randn(BS, A, E, generator=g).cuda(), torch.randn(BS, A, 11, generator=g).cuda()
    cached_f, cached_a = torch.randn(BS, T, E, generator=g).cuda(), torch.randn(BS, T, 11, generator=g).cuda()
    index = torch.stack([torch.randperm(A, generator=g)[: A - T] for _ in range(BS)]).int().cuda()
    mask = _u8((1, 0, 1))   # the bank's validity mask: stream 1's history is masked out ...
    act = [0, 2]
    full_iid = iid.clone()
    out_f, out_a = _merge(full_iid, cur_f, cur_a, cached_f, cached_a, index, mask, BS, active=_u8((1, 0, 1)))   # ... and it is paused
    sub_iid = iid[act].clone()
    sub_f, sub_a = _merge(sub_iid, cur_f[act].contiguous(), cur_a[act].contiguous(), cached_f[act].contiguous(),
                          cached_a[act].contiguous(), index[act].contiguous(), mask[act].contiguous(), 2)
    sib_iid = iid.clone()
    _merge(sib_iid, cur_f, cur_a, cached_f, cached_a, index, mask, BS)
    all_iid = iid.clone()
    _merge(all_iid, cur_f, cur_a, cached_f, cached_a, index, mask, BS, active=_u8((1, 1, 1)))
    torch.cuda.synchronize()
    assert torch.equal(full_iid[1], iid[1]) and bool((iid[1] >= 0).all())
    assert bool((sib_iid[1] == -1).all()) and torch.equal(all_iid, sib_iid)   # what the sibling does to it
    assert torch.equal(full_iid[act], sub_iid) and torch.equal(out_f[act], sub_f) and torch.equal(out_a[act], sub_a)


# ---------------------------------------------------------------------------------------------------------------- allocation
CAMS = 6


def _alloc(anchor, proj, per_stream, active=None, use_active_entry=True):
    L, lib, P, S = _lib()
    bs = anchor.shape[0]
    dev, slots = "cuda", bs * per_stream
    o = dict(flag=torch.full((bs, CAMS, A), 9, dtype=torch.uint8, device=dev), sel=torch.empty(bs, CAMS, A, 2, device=dev),
             depth=torch.empty(bs, CAMS, A, device=dev), count=torch.full((bs, CAMS), -5, dtype=torch.int32, device=dev),
             order=torch.zeros(bs, CAMS, A, dtype=torch.int32, device=dev),
             group_start=torch.full((bs * CAMS + 1,), -5, dtype=torch.int32, device=dev),
             overflow=torch.full((1,), -5, dtype=torch.int32, device=dev), pts=torch.full((slots, 2), -5.0, device=dev),
             d2=torch.full((slots,), -5.0, device=dev), q2a=torch.full((slots,), -5, dtype=torch.int32, device=dev),
             ctr=torch.full((slots,), -5, dtype=torch.int32, device=dev), a2q=torch.full((bs, A, CAMS), -5, dtype=torch.int32, device=dev),
             cam=torch.full((slots,), -5, dtype=torch.int32, device=dev))
    args = [P(o[k]) for k in ("flag", "sel", "depth", "count", "order", "group_start", "overflow", "pts", "d2", "q2a", "ctr", "a2q", "cam")]
    args += [P(anchor), P(proj), bs, A, CAMS, per_stream, 704.0, 256.0, 35.0, 35.0, 10.0]
    if use_active_entry:
        L.check(lib.simpb_alloc_ragged_active(*args, P(active) if active is not None else None, S()), "alloc_ragged_active")
    else:
        L.check(lib.simpb_alloc_ragged(*args, S()), "alloc_ragged")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _anchors(g):
    anchor = torch.from_numpy(synth.anchors(A)).float()[None].repeat(BS, 1, 1)
    anchor[..., :2] += torch.randn(BS, A, 2, generator=g) * 3.0
    return anchor


def _check_against_sub_batch(full, sub, act, per_stream):
    gs, sg = full["group_start"], sub["group_start"]
    live = int(sg[len(act) * CAMS])
    assert int(gs[BS * CAMS]) == live > 0                      # m_live of the 2D operators: the active streams' slots only
    for sb, b in enumerate(act):
        assert np.array_equal(gs[b * CAMS:(b + 1) * CAMS + 1], sg[sb * CAMS:(sb + 1) * CAMS + 1])
        assert np.array_equal(full["count"][b], sub["count"][sb]) and np.array_equal(full["flag"][b], sub["flag"][sb])
        assert np.array_equal(full["a2q"][b], sub["a2q"][sb])   # slot numbers are the sub-batch's: live slots first
    sub_stream = np.asarray(act)
    sq, sc = sub["q2a"], sub["cam"]
    want_q2a = np.where(sq >= 0, sub_stream[np.maximum(sq, 0) // A] * A + np.maximum(sq, 0) % A, -1)
    want_cam = np.where(sc >= 0, sub_stream[np.maximum(sc, 0) // CAMS] * CAMS + np.maximum(sc, 0) % CAMS, -1)
    n = len(act) * per_stream
    assert np.array_equal(full["q2a"][:n], want_q2a) and np.array_equal(full["cam"][:n], want_cam)
    for k in ("pts", "d2", "ctr"):
        assert np.array_equal(full[k][:n], sub[k]), k
    # the slots the sub-batch does not have are capacity slots
    assert (full["q2a"][n:] == -1).all() and (full["cam"][n:] == -1).all() and (full["ctr"][n:] == 0).all()
    assert (full["pts"][n:] == 0).all() and (full["d2"][n:] == 0).all()


def test_allocation_gives_a_paused_stream_no_slots_and_moves_the_others_down():
    g = torch.Generator().manual_seed(2)
    anchor = _anchors(g)
    anchor[1] = float("nan")
    anchor = anchor.cuda()
    proj = synth.frame_metas(BS, 0)["projection_mat"].cuda().contiguous()
    per_stream, act = 128, [0, 2]
    full = _alloc(anchor, proj, per_stream, active=_u8((1, 0, 1)))
    sub = _alloc(anchor[act].contiguous(), proj[act].contiguous(), per_stream, use_active_entry=False)
    assert (full["count"][1] == 0).all() and (full["flag"][1] == 0).all() and (full["a2q"][1] == -1).all()
    assert (np.diff(full["group_start"][CAMS:2 * CAMS + 1]) == 0).all()   # stream 1's six groups are empty
    assert int(full["overflow"][0]) == 0 == int(sub["overflow"][0])
    _check_against_sub_batch(full, sub, act, per_stream)
    # NULL mask: the entry point without one, table by table
    a = _alloc(anchor[act].contiguous(), proj[act].contiguous(), per_stream, active=None)
    for k in a:
        assert np.array_equal(a[k], sub[k], equal_nan=a[k].dtype.kind == "f"), k


def test_a_paused_stream_cannot_raise_overflow():
    """Stream 1 sees every anchor, streams 0 and 2 only a few: with a capacity between the two, the batch overflows when
    stream 1 takes part and does not when it is paused."""
    g = torch.Generator().manual_seed(4)
    anchor = _anchors(g)
    anchor[0, 12:, 2] = 1e4   # far above every camera: no corner and no centre inside an image
    anchor[2, 12:, 2] = 1e4
    anchor = anchor.cuda()
    proj = synth.frame_metas(BS, 0)["projection_mat"].cuda().contiguous()
    need = _alloc(anchor, proj, 512, active=None)["count"].sum(axis=1)
    per_stream = int(max(need[0], need[2]))
    assert need[1] > per_stream > 0, need
    act = [0, 2]
    assert int(_alloc(anchor, proj, per_stream, active=_u8((1, 1, 1)))["overflow"][0]) == 1
    full = _alloc(anchor, proj, per_stream, active=_u8((1, 0, 1)))
    sub = _alloc(anchor[act].contiguous(), proj[act].contiguous(), per_stream, use_active_entry=False)
    assert int(full["overflow"][0]) == 0 and (full["count"][1] == 0).all() and (full["a2q"][1] == -1).all()
    _check_against_sub_batch(full, sub, act, per_stream)
