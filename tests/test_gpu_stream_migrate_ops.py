"""GPU: the two entry points that move one stream of the bank (csrc/bank.hip simpb_bank_export_stream /
simpb_bank_import_stream) through ctypes, and InstanceBank.export_stream / import_stream on their HIP route, against the numpy
statement of the stream record in tests/stream_state_ref.py -- byte for byte: the kernels move bits."""
import ctypes

import numpy as np
import pytest
import torch

from tests import stream_state_ref as R

pytestmark = pytest.mark.gpu

BS = 3
CANARY = 64            # bytes in front of and behind the record
STATE = ("confidence", "cached_anchor", "cached_feature", "instance_id")


def _lib():
    from simpb_amd import _lib as L
    from simpb_amd.plugin.ops import _ptr, _stream
    return L, L.lib(), _ptr, _stream


def _dev(state):
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in state.items()}


def _host(dev):
    torch.cuda.synchronize()
    return {k: dev[k].cpu().numpy() for k in STATE}


def _same(a, b):
    return all(R.bits(a[k]) == R.bits(b[k]) for k in STATE)


def _export(dev, b, dims, blob):
    L, lib, ptr, stream = _lib()
    T, N, C, D = dims
    return lib.simpb_bank_export_stream(ptr(blob), ptr(dev["confidence"]), ptr(dev["cached_feature"]), ptr(dev["cached_anchor"]),
                                        ptr(dev["instance_id"]), b, BS, T, N, C, D, stream())


def _import(dev, prev_id, b, dims, blob):
    L, lib, ptr, stream = _lib()
    T, N, C, D = dims
    return lib.simpb_bank_import_stream(ptr(dev["confidence"]), ptr(dev["cached_feature"]), ptr(dev["cached_anchor"]),
                                        ptr(dev["instance_id"]), ptr(prev_id), ptr(blob), b, BS, T, N, C, D, stream())


def _arena(size, offset):
    """A device buffer of random bytes with a record-sized window at 16-byte alignment + offset -> (arena, window, copy)."""
    g = torch.Generator().manual_seed(size + offset)
    arena = torch.randint(0, 256, (CANARY + size + CANARY + 16,), dtype=torch.uint8, generator=g).cuda()
    start = CANARY + (-(arena.data_ptr() + CANARY) % 16) + offset
    window = arena[start: start + size]
    assert window.data_ptr() % 16 == offset
    return arena, window, start, arena.cpu().numpy().copy()


@pytest.mark.parametrize("offset", [0, 8])
@pytest.mark.parametrize("dims", R.SHAPES)
def test_export_and_import_kernels_equal_the_numpy_model_byte_for_byte(dims, offset):
    """Every slot of a bank of random bits (NaN payloads, infinities, denormals, -0.0) out into a record at a 16-byte
    aligned address and at one 8 bytes off, and into every slot of another bank: the record, the imported rows and prev_id are
    the model's; the bytes around the record, the source bank and every other stream's rows of the destination keep theirs;
    import followed by export reproduces the record."""
    src_state, dst_state = R.random_state(BS, *dims, seed=11), R.random_state(BS, *dims, seed=12)
    src = _dev(src_state)
    size = R.size(*dims)
    for b in range(BS):
        want = R.pack(src_state, b)
        arena, window, start, before = _arena(size, offset)
        assert _export(src, b, dims, window) == 0
        after = arena.cpu().numpy()
        assert after[start: start + size].tobytes() == want.tobytes(), (dims, b, offset)
        assert after[:start].tobytes() == before[:start].tobytes() and after[start + size:].tobytes() == before[start + size:].tobytes()
        assert _same(_host(src), src_state)
        for slot in range(BS):
            dst = _dev(dst_state)
            prev_id = torch.tensor([3], dtype=torch.long, device="cuda")
            assert _import(dst, prev_id, slot, dims, window) == 0
            want_state, want_prev = R.unpack(dst_state, 3, slot, want)
            assert _same(_host(dst), want_state), (dims, b, slot, offset)
            assert int(prev_id) == want_prev
            assert arena.cpu().numpy().tobytes() == after.tobytes()                       # the record is only read
            again = torch.zeros(size, dtype=torch.uint8, device="cuda")
            assert _export(dst, slot, dims, again) == 0
            assert again.cpu().numpy().tobytes() == want.tobytes()
            assert _import(dst, prev_id, slot, dims, window) == 0                          # idempotent, the floor included
            assert _same(_host(dst), want_state) and int(prev_id) == want_prev


@pytest.mark.parametrize("ids,prev,want", [
    ([5, -1, 9, 2], 20, 20), ([5, -1, 19, 2], 20, 20), ([5, -1, 20, 2], 20, 21), ([5, 4000, -1, 2], 20, 4001),
    ([-1, -1, -1, -1], 20, 20), ([-1, -1, -1, -1], 0, 0), ([2 ** 33 + 5, 7, -1, 2 ** 33 + 4], 20, 2 ** 33 + 6),
    ([2 ** 33 + 5, 7, -1, 1], 2 ** 40, 2 ** 40),
])
def test_import_raises_the_id_counter_on_the_device(ids, prev, want):
    """The cases of tests/test_stream_migrate_host.py; the largest id sits in a row longer than one workgroup pass (N = 600
    ids over 256 threads) at its first, a middle and its last position."""
    from simpb_amd.plugin.instance_bank import record_header
    dims = (5, 600, 32, 11)
    for at in (0, 300, 599):
        state = R.random_state(BS, *dims, seed=13)
        row = np.full(600, -1, np.int64)
        rest = sorted(ids)[:-1]
        row[[(at + 7 * (i + 1)) % 600 for i in range(len(rest))]] = rest
        row[at] = max(ids)
        state["instance_id"][1] = row
        src = _dev(state)
        blob = torch.zeros(R.size(*dims), dtype=torch.uint8, device="cuda")
        assert _export(src, 1, dims, blob) == 0
        assert record_header(blob)["largest_id"] == max(ids)
        dst = _dev(R.random_state(BS, *dims, seed=14))
        prev_id = torch.tensor([prev], dtype=torch.long, device="cuda")
        assert _import(dst, prev_id, 2, dims, blob) == 0
        assert int(prev_id) == want == R.unpack(state, prev, 2, blob.cpu().numpy())[1]
        assert R.bits(_host(dst)["instance_id"][2]) == R.bits(row)


def test_bad_arguments_return_einval():
    dims = (5, 7, 256, 11)
    dev = _dev(R.random_state(BS, *dims, seed=15))
    before = _host(dev)
    blob = torch.zeros(R.size(*dims) + 16, dtype=torch.uint8, device="cuda")
    prev_id = torch.zeros(1, dtype=torch.long, device="cuda")
    assert _export(dev, 0, dims, blob) == 0 and _import(dev, prev_id, 0, dims, blob) == 0
    for b in (-1, BS, BS + 5):
        assert _export(dev, b, dims, blob) == 1 and _import(dev, prev_id, b, dims, blob) == 1
    for i in range(4):
        bad = list(dims)
        for v in (0, -3):
            bad[i] = v
            assert _export(dev, 0, tuple(bad), blob) == 1 and _import(dev, prev_id, 0, tuple(bad), blob) == 1
    L, lib, ptr, stream = _lib()
    null = ctypes.c_void_p(0)
    T, N, C, D = dims
    p = [ptr(blob), ptr(dev["confidence"]), ptr(dev["cached_feature"]), ptr(dev["cached_anchor"]), ptr(dev["instance_id"])]
    for i in range(5):
        args = list(p)
        args[i] = null
        assert lib.simpb_bank_export_stream(*args, 0, BS, T, N, C, D, stream()) == 1
    q = [ptr(dev["confidence"]), ptr(dev["cached_feature"]), ptr(dev["cached_anchor"]), ptr(dev["instance_id"]), ptr(prev_id), ptr(blob)]
    for i in range(6):
        args = list(q)
        args[i] = null
        assert lib.simpb_bank_import_stream(*args, 0, BS, T, N, C, D, stream()) == 1
    assert lib.simpb_bank_export_stream(ptr(blob[4:]), *p[1:], 0, BS, T, N, C, D, stream()) == 1   # a record at 4 bytes off
    zero_batch = lib.simpb_bank_export_stream(*p, 0, 0, T, N, C, D, stream())
    assert zero_batch == 1
    assert _same(_host(dev), before)   # (the one valid import above rewrote slot 0 with its own rows)
    assert int(prev_id) == max(0, int(before["instance_id"][0].max()) + 1)


def test_the_bank_methods_take_the_hip_route_on_the_device():
    """InstanceBank.export_stream / import_stream with the persistent state on the GPU: the launches, equal to the PyTorch
    statement (fused=False) and to the model; a wrong record is refused before anything is written."""
    from simpb_amd.plugin.instance_bank import InstanceBank
    dims = T, N, C, D = (37, 70, 32, 11)
    state = R.random_state(BS, *dims, seed=16)

    def bank(st, prev):
        b = InstanceBank(num_anchor=N, embed_dims=C, anchor=np.zeros((N, D), np.float32), num_temp_instances=T)
        b.enable_static(BS, torch.device("cuda"))
        for k in STATE:
            b._static[k].copy_(torch.from_numpy(st[k].copy()))   # (bit-preserving: a same-dtype copy)
        b._static["prev_id"].fill_(prev)
        return b

    src = bank(state, 9)
    want = R.pack(state, 1)
    rec = src.export_stream(1)
    assert rec.is_cuda and rec.cpu().numpy().tobytes() == want.tobytes()
    assert src.export_stream(1, fused=False).cpu().numpy().tobytes() == want.tobytes()
    other = R.random_state(BS, *dims, seed=17)
    for fused in (True, False, None):
        dst = bank(other, 2)
        dst.import_stream(2, rec, fused=fused)
        want_state, want_prev = R.unpack(other, 2, 2, want)
        assert _same(_host(dst._static), want_state) and int(dst._static["prev_id"]) == want_prev, fused
        assert dst.has_history and dst.confidence is dst._static["confidence"]
    dst = bank(other, 2)
    broken = rec.clone()
    broken[0] = 0
    with pytest.raises(ValueError, match="magic"):
        dst.import_stream(2, broken)
    with pytest.raises(ValueError, match="device"):
        dst.import_stream(2, rec.cpu())
    assert _same(_host(dst._static), other) and int(dst._static["prev_id"]) == 2
