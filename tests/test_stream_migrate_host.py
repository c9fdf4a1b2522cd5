"""CPU: the host side of moving a live stream (InstanceBank.export_stream / import_stream in their PyTorch statement,
runner.StreamState, runner.adopt_metas, runner.normalise_adopt and the runners' refusals) against the numpy statement of the
stream record in tests/stream_state_ref.py."""
import numpy as np
import pytest
import torch

from tests import stream_restart_schedule as S
from tests import stream_state_ref as R

BS = 3


def _bank(T, N, C, D, state=None, prev_id=0):
    """An InstanceBank of these sizes with its persistent state on the host, holding `state` (numpy, stream_state_ref)."""
    from simpb_amd.plugin.instance_bank import InstanceBank
    assert D == 11
    bank = InstanceBank(num_anchor=N, embed_dims=C, anchor=np.zeros((N, D), np.float32), num_temp_instances=T)
    bank.enable_static(BS, "cpu")
    if state is not None:
        _set(bank, state, prev_id)
    return bank


def _set(bank, state, prev_id):
    for k, v in state.items():
        raw = torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1).copy())
        bank._static[k].view(-1).view(torch.uint8).copy_(raw)
    bank._static["prev_id"].fill_(int(prev_id))


def _get(bank):
    return {k: bank._static[k].numpy().copy() for k in ("confidence", "cached_anchor", "cached_feature", "instance_id")}


# ---------------------------------------------------------------------------------------------------------- 1. the layout
def test_the_layout_is_a_pure_function_of_the_sizes():
    from simpb_amd.plugin.instance_bank import RECORD_HEADER, RECORD_MAGIC, RECORD_VERSION, record_layout
    assert (RECORD_MAGIC, RECORD_VERSION, RECORD_HEADER) == (R.MAGIC, R.VERSION, R.HEADER)
    for dims in R.SHAPES + [(600, 900, 256, 11), (1, 1, 4, 11)]:
        lay = record_layout(*dims)
        assert lay == R.offsets(*dims) and lay["size"] == R.size(*dims)
        assert all(v % 16 == 0 for v in lay.values())
    T, N, C, D = 37, 70, 32, 11
    assert R.size(T, N, C, D) == 64 + 160 + 1632 + 4736 + 560   # 148 -> 160 and 1628 -> 1632: two sections are padded
    with pytest.raises(ValueError):
        record_layout(0, 7, 256, 11)


@pytest.mark.parametrize("dims", R.SHAPES)
def test_pytorch_statement_equals_the_numpy_model_byte_for_byte(dims):
    """Export of every slot, the header fields, import into every slot of another bank (the neighbours' rows keep their bytes,
    NaN patterns included), and import followed by export reproduces the record."""
    from simpb_amd.plugin.instance_bank import record_header
    T, N, C, D = dims
    src_state, dst_state = R.random_state(BS, *dims, seed=1), R.random_state(BS, *dims, seed=2)
    src = _bank(*dims, src_state, prev_id=17)
    for b in range(BS):
        want = R.pack(src_state, b)
        got = src.export_stream(b)
        assert got.dtype == torch.uint8 and got.numel() == R.size(*dims)
        assert got.numpy().tobytes() == want.tobytes(), (dims, b)
        out = torch.full((R.size(*dims),), 0xAB, dtype=torch.uint8)
        assert src.export_stream(b, out=out) is out and out.numpy().tobytes() == want.tobytes()   # (padding is written too)
        h = record_header(got)
        ids = src_state["instance_id"][b]
        assert h == dict(magic=R.MAGIC, version=R.VERSION, num_temp=T, num_anchor=N, embed_dims=C, anchor_dims=D,
                         largest_id=max(-1, int(ids.max())))
        assert all(R.bits(v) == R.bits(src_state[k]) for k, v in _get(src).items()) and int(src._static["prev_id"]) == 17
        for slot in range(BS):
            dst = _bank(*dims, dst_state, prev_id=3)
            dst.import_stream(slot, got)
            want_state, want_prev = R.unpack(dst_state, 3, slot, want)
            have = _get(dst)
            assert all(R.bits(have[k]) == R.bits(want_state[k]) for k in have), (dims, b, slot)
            assert int(dst._static["prev_id"]) == want_prev
            assert dst.export_stream(slot).numpy().tobytes() == want.tobytes()
            assert dst.has_history and dst.cached_feature is dst._static["cached_feature"]


@pytest.mark.parametrize("ids,prev,want", [
    ([5, -1, 9, 2], 20, 20),                       # every id below the counter
    ([5, -1, 19, 2], 20, 20),                      # the largest id is the last one issued: the counter already clears it
    ([5, -1, 20, 2], 20, 21),                      # equal to the counter: that id would be issued again
    ([5, 4000, -1, 2], 20, 4001),                  # above
    ([-1, -1, -1, -1], 20, 20),                    # no id at all
    ([-1, -1, -1, -1], 0, 0),
    ([2 ** 33 + 5, 7, -1, 2 ** 33 + 4], 20, 2 ** 33 + 6),   # beyond 32 bits
    ([2 ** 33 + 5, 7, -1, 1], 2 ** 40, 2 ** 40),
])
def test_import_raises_the_id_counter_to_clear_the_record(ids, prev, want):
    dims = (5, 7, 256, 11)
    state = R.random_state(BS, *dims, seed=3)
    state["instance_id"][1] = np.array(ids + [-1] * (7 - len(ids)), np.int64)
    rec = _bank(*dims, state).export_stream(1)
    for slot in (0, 2):
        dst = _bank(*dims, R.random_state(BS, *dims, seed=4), prev_id=prev)
        dst.import_stream(slot, rec)
        assert int(dst._static["prev_id"]) == want == R.unpack(state, prev, slot, rec.numpy())[1]
        dst.import_stream(slot, rec)   # idempotent, the floor included
        assert int(dst._static["prev_id"]) == want


def test_records_and_banks_that_do_not_match_are_refused_in_words():
    from simpb_amd.plugin.instance_bank import InstanceBank
    dims = (5, 7, 256, 11)
    bank = _bank(*dims, R.random_state(BS, *dims, seed=5))
    rec = bank.export_stream(0)
    before = _get(bank)

    def bad(change, match):
        r = rec.clone()
        change(r)
        with pytest.raises(ValueError, match=match):
            bank.import_stream(1, r)

    bad(lambda r: r[0:4].zero_(), "magic")
    bad(lambda r: r[4:8].copy_(torch.tensor([2, 0, 0, 0], dtype=torch.uint8)), "version")
    bad(lambda r: r[8:12].copy_(torch.tensor([6, 0, 0, 0], dtype=torch.uint8)), r"\(T, N, C, D\)")
    with pytest.raises(ValueError, match="bytes"):
        bank.import_stream(1, rec[:-16].clone())
    with pytest.raises(ValueError, match="header"):
        bank.import_stream(1, rec[:10].clone())
    with pytest.raises(ValueError, match=r"\(T, N, C, D\)"):
        _bank(37, 70, 32, 11).import_stream(0, rec)
    with pytest.raises(ValueError, match="stream 3"):
        bank.export_stream(3)
    with pytest.raises(ValueError, match="out"):
        bank.export_stream(0, out=torch.zeros(10, dtype=torch.uint8))
    assert all(R.bits(v) == R.bits(before[k]) for k, v in _get(bank).items())   # nothing was written
    eager = InstanceBank(num_anchor=7, embed_dims=256, anchor=np.zeros((7, 11), np.float32), num_temp_instances=5)
    with pytest.raises(ValueError, match="enable_static"):   # the HIP route without persistent state
        eager.export_stream(0, fused=True)
    with pytest.raises(ValueError, match="enable_static"):
        eager.import_stream(0, rec, fused=True)
    with pytest.raises(ValueError, match="no temporal state"):
        eager.export_stream(0)
    with pytest.raises(ValueError, match="GPU"):               # ... and with it on the host
        bank.export_stream(0, fused=True)


def test_bad_arguments_return_einval_without_a_device():
    """Argument validation runs before any HIP call (as tests/test_capi.py checks for the samplers)."""
    import ctypes
    from simpb_amd import _lib
    h = _lib.lib()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)
    sizes = (5, 7, 256, 11)
    for i in range(5):
        ptrs = [p] * 5
        ptrs[i] = null
        assert h.simpb_bank_export_stream(*ptrs, 0, 3, *sizes, null) == 1
    for i in range(6):
        ptrs = [p] * 6
        ptrs[i] = null
        assert h.simpb_bank_import_stream(*ptrs, 0, 3, *sizes, null) == 1
    for stream, bs in ((-1, 3), (3, 3), (0, 0), (0, -2)):
        assert h.simpb_bank_export_stream(p, p, p, p, p, stream, bs, *sizes, null) == 1
        assert h.simpb_bank_import_stream(p, p, p, p, p, p, stream, bs, *sizes, null) == 1
    for i in range(4):
        for v in (0, -1):
            bad = list(sizes)
            bad[i] = v
            assert h.simpb_bank_export_stream(p, p, p, p, p, 0, 3, *bad, null) == 1
            assert h.simpb_bank_import_stream(p, p, p, p, p, p, 0, 3, *bad, null) == 1
    off = ctypes.c_void_p(68)   # a record that is not at a multiple of 8 bytes
    assert h.simpb_bank_export_stream(off, p, p, p, p, 0, 3, *sizes, null) == 1
    assert h.simpb_bank_import_stream(p, p, p, p, p, off, 0, 3, *sizes, null) == 1


# ------------------------------------------------------------------------------------------------------- 2. StreamState
def _state(dims=(5, 7, 256, 11), seed=6, slot=1):
    from simpb_amd.runner import StreamState
    bank = _bank(*dims, R.random_state(BS, *dims, seed=seed))
    pose = np.arange(16, dtype=np.float64).reshape(4, 4) + 0.1
    return StreamState(bank.export_stream(slot), bank.record_dims(), pose, np.linalg.inv(pose + np.eye(4) * 50), 1234.5678901234)


def test_stream_state_survives_a_byte_string():
    from simpb_amd.runner import StreamState
    st = _state()
    data = st.to_bytes()
    assert isinstance(data, bytes) and len(data) == R.size(*st.dims) + 33 * 8
    back = StreamState.from_bytes(data)
    assert back.dims == st.dims and back.sealed and back.record.device.type == "cpu"
    assert back.record.numpy().tobytes() == st.record.numpy().tobytes()
    assert back.T_global.tobytes() == st.T_global.tobytes() and back.T_global_inv.tobytes() == st.T_global_inv.tobytes()
    assert back.timestamp == st.timestamp and back.to_bytes() == data
    assert back.T_global.dtype == np.float64 and set(back.img_meta()) == {"T_global", "T_global_inv", "timestamp"}
    assert st.to("cpu") is st
    for cut in (0, 10, 64, len(data) - 1, len(data) - 264):
        with pytest.raises(ValueError):
            StreamState.from_bytes(data[:cut])
    with pytest.raises(ValueError, match="bytes"):
        StreamState.from_bytes(data + b"\0" * 16)
    with pytest.raises(ValueError, match="magic"):
        StreamState.from_bytes(b"\1\2\3\4" + data[4:])
    with pytest.raises(ValueError, match="version"):
        StreamState.from_bytes(data[:4] + b"\7\0\0\0" + data[8:])
    with pytest.raises(ValueError):
        StreamState.from_bytes(data[:8] + b"\6\0\0\0" + data[12:])   # another T: another size
    with pytest.raises(ValueError):
        StreamState(st.record[:-16], st.dims, st.T_global, st.T_global_inv, 0.0)


def test_an_unsealed_state_cannot_be_used():
    from simpb_amd.runner import normalise_adopt
    st = _state()
    st._sealed = False
    for use in (lambda: st.record, st.to_bytes, lambda: st.to("cpu"), st.wait, lambda: normalise_adopt({0: st}, BS, st.dims)):
        with pytest.raises(RuntimeError, match="results have not been returned"):
            use()
    st._sealed = True
    assert normalise_adopt({0: st}, BS, st.dims) == {0: st}


# ------------------------------------------------------------------------------------------------------ 3. staged motion
def test_adopt_metas_is_pure_and_replaces_only_the_adopted_entries():
    from simpb_amd.runner import FrameInputs, adopt_metas, stream_motion
    _, prev = S.frame(2)
    _, cur = S.frame(3, restarts=False)
    _, home = S.frame(1)   # the adopted stream's last active frame was step 1, elsewhere
    m = home["img_metas"][2]
    st = _state()
    st.T_global, st.T_global_inv, st.timestamp = np.array(m["T_global"], np.float64), np.array(m["T_global_inv"], np.float64), float(m["timestamp"])
    before = [dict(e) for e in prev["img_metas"]]
    listed = prev["img_metas"]
    staged = adopt_metas(dict(img_metas=prev["img_metas"]), {2: st})
    assert prev["img_metas"] is listed and all(o.keys() == n.keys() and all(o[k] is n[k] for k in o)
                                               for o, n in zip(before, prev["img_metas"]))
    assert staged["img_metas"] is not prev["img_metas"]
    assert staged["img_metas"][0] is prev["img_metas"][0] and staged["img_metas"][1] is prev["img_metas"][1]
    assert set(staged["img_metas"][2]) == {"T_global", "T_global_inv", "timestamp"}
    t, dt = stream_motion(cur, staged)
    t_home, dt_home = stream_motion(cur, dict(img_metas=[prev["img_metas"][0], prev["img_metas"][1], m]))
    assert t.tobytes() == t_home.tobytes() and dt.tobytes() == dt_home.tobytes() and dt[2] == np.float32(1.0)
    # the previous occupant's pose and time stamp as NaN: the same bytes
    bad = np.full((4, 4), np.nan)
    poisoned = [prev["img_metas"][0], prev["img_metas"][1], dict(prev["img_metas"][2], T_global=bad, T_global_inv=bad, timestamp=float("nan"))]
    t2, dt2 = stream_motion(cur, adopt_metas(dict(img_metas=poisoned), {2: st}))
    assert t2.tobytes() == t.tobytes() and dt2.tobytes() == dt.tobytes()
    with pytest.raises(ValueError):
        adopt_metas(dict(img_metas=prev["img_metas"]), {3: st})
    inp = FrameInputs(S.BS, S.CAMS, "cpu", time_step=(2.0, 0.5))
    inp.fill(cur, staged, None, None)
    assert inp.host["dt"].tolist() == [0.5, 0.5, 1.0] and not inp.restarting


# ----------------------------------------------------------------------------------------------------------- 4. refusals
def test_adoptions_are_normalised_and_refused_by_the_rules():
    from simpb_amd.runner import normalise_adopt
    st = _state()
    dims = st.dims
    assert normalise_adopt(None, BS, dims) is None and normalise_adopt({}, BS, dims) is None
    assert list(normalise_adopt({2: st, 0: st}, BS, dims)) == [0, 2]
    assert normalise_adopt({0: st}, 1, dims, independent=False) == {0: st}             # a batch of one always is independent
    for slot in (-1, 3, 1.5, "a"):
        with pytest.raises((ValueError, TypeError)):
            normalise_adopt({slot: st}, BS, dims)
    with pytest.raises(ValueError, match="StreamState"):
        normalise_adopt({0: st.record}, BS, dims)
    with pytest.raises(ValueError, match=r"\(T, N, C, D\)"):
        normalise_adopt({0: st}, BS, (64, 128, 256, 11))
    with pytest.raises(ValueError, match="paused and adopted"):
        normalise_adopt({1: st}, BS, dims, active=(True, False, True))
    assert normalise_adopt({1: st}, BS, dims, active=(False, True, True), restart=(False, False, True)) == {1: st}
    with pytest.raises(ValueError, match="adopted and restarted"):
        normalise_adopt({1: st}, BS, dims, restart=(False, True, False))
    with pytest.raises(ValueError, match="independent_streams"):
        normalise_adopt({1: st}, BS, dims, independent=False)
    with pytest.raises(NotImplementedError, match="already in"):
        normalise_adopt({0: st}, 1, dims, supported=False)
    assert normalise_adopt({}, 1, dims, supported=False) is None


class _NoDetector(torch.nn.Module):
    def __init__(self, head):
        super().__init__()
        self.head = head

    def extract_feat(self, img):
        raise AssertionError("a refused call runs nothing")


def _cpu_runner(independent=True, cls=None):
    from simpb_amd import runner
    from tests.helpers import build_product_head
    spec = dict(num_anchor=128, num_temp=64, num_output=32)
    model = _NoDetector(build_product_head(spec, device="cpu"))
    cls = cls or runner.FrameRunner
    return cls(model, BS, (S.WH[1], S.WH[0]), capacity=256, device=torch.device("cpu"), use_graph=False,
               independent_streams=independent)


def test_the_runners_refuse_before_anything_runs():
    from simpb_amd.runner import FrameRunner, PipelinedRunner, SplitPipelinedRunner, StreamState
    r = _cpu_runner()
    dims = r.head.instance_bank.record_dims()
    assert dims == (64, 128, 256, 11)
    _, metas = S.frame(0)
    good = StreamState(torch.zeros(R.size(*dims), dtype=torch.uint8), dims, np.eye(4), np.eye(4), 0.0)
    # exports: nothing decoded yet, a stream out of range
    for s, kind in ((0, ValueError), (3, ValueError), (-1, ValueError)):
        with pytest.raises(kind):
            r.export_stream(s)
    with pytest.raises(ValueError, match="nothing to export"):
        r.export_stream(1)
    r.decoded = [True] * BS
    padded = _cpu_runner(independent=False)
    padded.decoded = [True] * BS
    with pytest.raises(ValueError, match="independent_streams"):
        padded.export_stream(1)
    with pytest.raises(ValueError, match="independent_streams"):
        padded.step(padded.img, metas, adopt={1: good})
    # adoptions
    with pytest.raises(ValueError, match=r"\(T, N, C, D\)"):
        r.step(r.img, metas, adopt={1: _state()})
    with pytest.raises(ValueError, match="slot"):
        r.step(r.img, metas, adopt={3: good})
    with pytest.raises(ValueError, match="adopted and restarted"):
        r.step(r.img, metas, adopt={1: good}, restart=[False, True, False])
    with pytest.raises(ValueError, match="paused and adopted"):
        r.step(r.img, metas, adopt={1: good}, active=[True, False, True])
    unsealed = StreamState(good.record, dims, np.eye(4), np.eye(4), 0.0, sealed=False)
    with pytest.raises(RuntimeError):
        r.step(r.img, metas, adopt={1: unsealed})
    assert r.prev_metas is None and "adopt" not in r.stats and not r.head.instance_bank.has_history   # nothing ran
    assert FrameRunner.SUPPORTS_RESTART and PipelinedRunner.SUPPORTS_RESTART and not SplitPipelinedRunner.SUPPORTS_RESTART
    probe = FrameRunner.__new__(SplitPipelinedRunner)   # (its constructor makes device streams: the class rule alone)
    probe.bs, probe.independent, probe.decoded = 1, False, [True]
    with pytest.raises(NotImplementedError, match="already in"):
        probe._check_export(0)


def test_a_first_frame_with_an_adoption_is_staged_warm_with_the_others_restarted():
    """_admit of a runner that has not decoded a frame: with an adoption the frame is staged against the adopted state's metas
    and the frame's own for every other slot, which are restarted; without one it is today's cold frame."""
    from simpb_amd.runner import StreamState, stream_motion
    r = _cpu_runner()
    dims = r.head.instance_bank.record_dims()
    _, home = S.frame(1)
    _, metas = S.frame(2, restarts=False)
    m = home["img_metas"][0]
    st = StreamState(torch.zeros(R.size(*dims), dtype=torch.uint8), dims, m["T_global"], m["T_global_inv"], m["timestamp"])
    mask, cams, out, img, flags, adopt, prev = r._admit(None, r.img, metas, None, None, None, None)
    assert (mask, cams, flags, adopt, prev) == (None, None, None, None, None) and "adopt" not in r.stats
    mask, cams, out, img, flags, adopt, prev = r._admit(None, r.img, metas, None, None, None, {0: st})
    assert mask is None and flags == (False, True, True) and list(adopt) == [0] and r.stats["adopt"] == 1
    assert prev["img_metas"][1] is metas["img_metas"][1] and prev["img_metas"][2] is metas["img_metas"][2]
    t, dt = stream_motion(metas, prev)
    assert dt.tolist() == [0.5, 0.0, 0.0]
    # every slot adopted: an ordinary warm frame
    flags = r._admit(None, r.img, metas, None, None, None, {0: st, 1: st, 2: st})[4]
    assert flags is None


# ------------------------------------------------------------------------------------------------- 5. the oracle's margins
def test_oracle_margins_of_the_moved_stream_stay_inside_the_cap():
    """The oracle alone on stream 1 of the schedule without restarts (the stream tests/test_gpu_stream_migrate.py moves at step
    3): the three margins of tests/test_gpu_stream_activity.py::_tie_evidence for the steps behind the move. The GPU
    comparison with the stay-at-home run excuses a miss only by a margin < 1e-4 and for at most ONE of those steps -- a
    condition the oracle's own numbers must leave room for: at most one step below 1e-4 here."""
    from oracle import simpb_ref as O
    from tests.helpers import build_product_head
    from tests.test_gpu_stream_activity import SPEC, _tie_evidence
    head = build_product_head(SPEC, device="cpu")
    params = {k: v.detach().cpu() for k, v in head.state_dict().items()}
    A, T, N = SPEC["num_anchor"], SPEC["num_temp"], SPEC["num_output"]
    torch.set_num_threads(16)
    chain = O.OracleHead(params, head.operation_order, A, T, N)
    tight = []
    with torch.no_grad():
        for step in range(S.STEPS):
            maps, metas = S.frame(step, restarts=False)
            fm = O.feature_maps_format(list(maps))
            one = S.one_stream(metas, 1)
            want = chain.forward([fm[0][1:2], fm[1], fm[2]], one)
            if step < 3:
                continue
            tie = _tie_evidence(want, one, T, N, [chain.p["instance_bank.anchor"][None]] + list(want["prediction"]))
            print("oracle margins of the moved stream: step %d: %s" % (step, tie))
            if min(tie.values()) < 1e-4:
                tight.append((step, tie))
    assert len(tight) <= 1, tight
