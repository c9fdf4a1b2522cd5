"""A numpy statement of the stream record (include/simpb_hip.h "stream record"): the layout, its size and the two moves.
Written from the layout table alone, without the package, so that the kernels, the PyTorch statement and the host parser are
all compared with something that shares no code with them. No GPU here.

    header         64 bytes: i32 magic, i32 version, i32 T, i32 N, i32 C, i32 D, i64 largest id (-1: none), zeros
    confidence     f32 [T]
    cached_anchor  f32 [T, D]
    cached_feature f32 [T, C]
    instance_id    i64 [N]

every section at a multiple of 16 bytes from the first byte, padding zero."""
import numpy as np

MAGIC, VERSION, HEADER = 0x42504D53, 1, 64
SHAPES = [(64, 128, 256, 11), (5, 7, 256, 11), (37, 70, 32, 11)]   # (T, N, C, D); the last: tails of 1 float, 3 floats, 0 ids


def _pad16(n):
    return -(-n // 16) * 16


def offsets(T, N, C, D):
    conf = HEADER
    anchor = conf + _pad16(4 * T)
    feature = anchor + _pad16(4 * T * D)
    ids = feature + _pad16(4 * T * C)
    return dict(confidence=conf, cached_anchor=anchor, cached_feature=feature, instance_id=ids, size=ids + _pad16(8 * N))


def size(T, N, C, D):
    return offsets(T, N, C, D)["size"]


def pack(state, b):
    """Stream b of state = dict(confidence [bs, T], cached_anchor [bs, T, D], cached_feature [bs, T, C], instance_id i64
    [bs, N]) (numpy) -> the record as a u8 array. Bits are moved, never numbers."""
    T, D = state["cached_anchor"].shape[1:]
    C, N = state["cached_feature"].shape[2], state["instance_id"].shape[1]
    off = offsets(T, N, C, D)
    out = np.zeros(off["size"], np.uint8)
    out[:24] = np.array([MAGIC, VERSION, T, N, C, D], "<i4").view(np.uint8)
    ids = np.ascontiguousarray(state["instance_id"][b], "<i8")
    out[24:32] = np.array([max(-1, int(ids.max()))], "<i8").view(np.uint8)
    for name in ("confidence", "cached_anchor", "cached_feature"):
        raw = np.ascontiguousarray(state[name][b]).view(np.uint8).ravel()
        assert state[name].dtype == np.float32
        out[off[name]: off[name] + raw.size] = raw
    out[off["instance_id"]: off["instance_id"] + 8 * N] = ids.view(np.uint8)
    return out


def unpack(state, prev_id, b, record):
    """The record into stream b of a COPY of `state` -> (state, prev_id) with prev_id = max(prev_id, 1 + largest id of the
    record's id row). The header is not looked at."""
    state = {k: v.copy() for k, v in state.items()}
    T, D = state["cached_anchor"].shape[1:]
    C, N = state["cached_feature"].shape[2], state["instance_id"].shape[1]
    off = offsets(T, N, C, D)
    assert record.dtype == np.uint8 and record.size == off["size"]
    for name, count in (("confidence", T), ("cached_anchor", T * D), ("cached_feature", T * C)):
        raw = record[off[name]: off[name] + 4 * count].copy()
        state[name][b] = raw.view(np.float32).reshape(state[name][b].shape)
    ids = record[off["instance_id"]: off["instance_id"] + 8 * N].copy().view("<i8")
    state["instance_id"][b] = ids
    return state, max(int(prev_id), int(ids.max()) + 1)


def random_state(bs, T, N, C, D, seed, specials=True):
    """A bank of random BITS (so NaN payloads, infinities and denormals are all there; specials adds some for sure) and an id
    table with -1 rows mixed in."""
    g = np.random.default_rng(seed)
    out = {}
    for name, shape in (("confidence", (bs, T)), ("cached_anchor", (bs, T, D)), ("cached_feature", (bs, T, C))):
        bits = g.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
        if specials:
            flat = bits.reshape(bs, -1)
            vals = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000], np.uint32)
            flat[:, : min(len(vals), flat.shape[1])] = vals[: flat.shape[1]]
        out[name] = bits.view(np.float32)
    ids = g.integers(0, 5000, size=(bs, N)).astype(np.int64)
    ids[g.random((bs, N)) < 0.4] = -1
    out["instance_id"] = ids
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()
