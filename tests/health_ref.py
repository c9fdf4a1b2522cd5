"""numpy model of camera health (include/simpb_hip.h, "Camera health"): the integer statistics of one image and the verdict per
(stream, camera). Every statistic is an integer that does not depend on the order of summation and the verdict is float64 with
one rounding per operation, so the device must reproduce all of it bit for bit. Written apart from simpb_amd/health.py, which
holds no arithmetic at all."""
import numpy as np

G = 8
BANDS, WORDS = 64, 26
DARK, BRIGHT, FLAT, FROZEN, FAIL_OPEN, NONFINITE = 1, 2, 4, 8, 16, 32
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix(z):
    """The splitmix64 finaliser on a uint64 array (multiplication mod 2^64)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def _q(x):
    """f16 [..., 3] -> (x * 2^24 as int64 with 0 for a non-finite x, the non-finite mask)."""
    x = x.astype(np.float64)
    bad = ~np.isfinite(x)
    q = np.where(bad, 0.0, x) * 2.0 ** 24
    assert (q == np.rint(q)).all()   # exact for every finite f16
    return q.astype(np.int64), bad


def _hash_terms(img):
    h, w = img.shape[:2]
    bits = np.ascontiguousarray(img[..., :3]).view(np.uint16).astype(np.uint64)
    idx = (np.arange(h * w * 3, dtype=np.uint64)).reshape(h, w, 3)
    return mix(bits | (idx << np.uint64(16)))


def edges(n):
    return [i * n // G for i in range(G + 1)]


def stats(img):
    """img f16 [H, W, 4] -> dict(S int64 [8, 8, 3], hash u64, nonfinite int). Channel 3 is not looked at."""
    img = np.asarray(img)
    assert img.dtype == np.float16 and img.ndim == 3 and img.shape[2] == 4
    h, w = img.shape[:2]
    q, bad = _q(img[..., :3])
    ys, xs = edges(h), edges(w)
    s = np.zeros((G, G, 3), np.int64)
    for i in range(G):
        for j in range(G):
            s[i, j] = q[ys[i]:ys[i + 1], xs[j]:xs[j + 1]].reshape(-1, 3).sum(0)
    with np.errstate(over="ignore"):
        hsh = _hash_terms(img).sum(dtype=np.uint64)
    return dict(S=s, hash=np.uint64(hsh), nonfinite=int(bad.sum()))


def partial_rows(img):
    """The partial rows the statistics launch leaves for one image: int64 [64, 26]. Band i * 8 + b: the b-th eighth of the
    rows of cell row i; a row: the band's S as [j * 3 + k], its hash part (as int64 bits), its non-finite count."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    q, bad = _q(img[..., :3])
    terms = _hash_terms(img)
    ys, xs = edges(h), edges(w)
    out = np.zeros((BANDS, WORDS), np.int64)
    for i in range(G):
        n = ys[i + 1] - ys[i]
        for b in range(G):
            r0, r1 = ys[i] + b * n // G, ys[i] + (b + 1) * n // G
            for j in range(G):
                out[i * G + b, j * 3:j * 3 + 3] = q[r0:r1, xs[j]:xs[j + 1]].reshape(-1, 3).sum(0)
            with np.errstate(over="ignore"):
                out[i * G + b, 24] = terms[r0:r1].sum(dtype=np.uint64).view(np.int64) if r1 > r0 else 0
            out[i * G + b, 25] = int(bad[r0:r1].sum())
    return out


def reduce_rows(rows):
    """Partial rows int64 [64, 26] -> the dict `stats` returns."""
    rows = np.asarray(rows, np.int64).reshape(G, G, WORDS)
    with np.errstate(over="ignore"):
        s = rows[..., :24].sum(1).reshape(G, G, 3)
        hsh = rows[..., 24].astype(np.uint64).sum(dtype=np.uint64)
    return dict(S=s, hash=np.uint64(hsh), nonfinite=int(rows[..., 25].sum()))


def pack_rows(st):
    """A `stats` dict -> partial rows with everything of cell row i in its first band (crafted statistics for the verdict)."""
    out = np.zeros((BANDS, WORDS), np.int64)
    for i in range(G):
        out[i * G, :24] = np.asarray(st["S"], np.int64)[i].reshape(24)
    out[0, 24] = np.array([st["hash"]], np.uint64).view(np.int64)[0]
    out[0, 25] = int(st["nonfinite"])
    return out


def levels(st, hw, mean, std):
    """(L, Lc [8, 8]) of one image's statistics, float64: per channel double(sum) / (double(pixels) * 2^24) * std + mean, then
    the mean of the three, each operation rounded once."""
    h, w = hw
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    s = np.asarray(st["S"], np.int64)

    def level(sum3, pixels):
        denom = np.asarray(pixels, np.float64)[..., None] * np.float64(2.0 ** 24)
        l = sum3.astype(np.float64) / denom * std + mean
        return ((l[..., 0] + l[..., 1]) + l[..., 2]) / np.float64(3.0)

    ys, xs = np.diff(edges(h)), np.diff(edges(w))
    with np.errstate(over="ignore"):
        total = s.sum((0, 1))
    return level(total, h * w), level(s, ys[:, None] * xs[None, :])


def new_state(bs, cams):
    return dict(prev_hash=np.zeros((bs, cams), np.uint64), repeats=np.zeros((bs, cams), np.uint32),
                frames=np.zeros((bs, cams), np.uint32))


def verdict(st, state, hw, mean, std, dark_below=16.0, bright_above=240.0, flat_below=2.0, frozen_after=2, act=True,
            cam_in=None, active=None):
    """st: [bs][cams] of `stats` dicts (None where the camera is not considered: they are not looked at); state: `new_state`
    dict, not modified. Returns (cam_out u8 [bs, cams], flags u8 [bs, cams], the state after the frame)."""
    bs, cams = state["frames"].shape
    cam_in = np.ones((bs, cams), bool) if cam_in is None else np.asarray(cam_in).astype(bool).reshape(bs, cams)
    active = np.ones(bs, bool) if active is None else np.asarray(active).astype(bool).reshape(bs)
    new = {k: v.copy() for k, v in state.items()}
    flags = np.zeros((bs, cams), np.uint8)
    cam_out = cam_in.astype(np.uint8)
    for s in range(bs):
        considered = [c for c in range(cams) if active[s] and cam_in[s, c]]
        for c in considered:
            x = st[s][c]
            level, cells = levels(x, hw, mean, std)
            f = 0
            if dark_below is not None and level < np.float64(dark_below):
                f |= DARK
            if bright_above is not None and level > np.float64(bright_above):
                f |= BRIGHT
            if flat_below is not None and cells.max() - cells.min() < np.float64(flat_below):
                f |= FLAT
            if x["nonfinite"] > 0:
                f |= NONFINITE
            same = new["frames"][s, c] > 0 and new["prev_hash"][s, c] == np.uint64(x["hash"])
            new["repeats"][s, c] = new["repeats"][s, c] + 1 if same else 0
            new["prev_hash"][s, c] = np.uint64(x["hash"])
            new["frames"][s, c] += 1
            if frozen_after is not None and new["repeats"][s, c] >= frozen_after:
                f |= FROZEN
            flags[s, c] = f
        fail_open = bool(considered) and all(flags[s, c] != 0 for c in considered)
        for c in considered:
            if fail_open:
                flags[s, c] |= FAIL_OPEN
            elif flags[s, c] != 0 and act:
                cam_out[s, c] = 0
    return cam_out, flags, new
