"""GPU: the *_live entry points (include/simpb_hip.h, "the backbone convolutions over the LIVE images of a batch only") against
the entry points without the suffix, every form forced.

Five images; maps of 8 x 22 and 16 x 44 (176 and 704 pixels per image: a multiple of no tile, so flat tiles straddle images
-- with the live sets {1, 3} and {0, 4} images that are no neighbours in memory -- and the resident 16-column tiles are
clipped); 64 and 128 channels. Every output buffer is pre-filled with a sentinel bit pattern, every input and residual row of
a dead image is NaN, and the entries of the table behind L name an image that is dead. One comparison of the WHOLE buffer,
byte for byte, against the sentinel buffer with the live images' rows of the full-batch launch (clean inputs, the same forced
variant) put in, says all three things at once: live rows are the full batch's bits, dead rows still hold the sentinel (so do
the token rows between levels), and the empty set leaves everything untouched."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 5
LIVE_SETS = ((0, 1, 2, 3, 4), (0,), (4,), (1, 3), (0, 4), ())
MAPS = ((8, 22), (16, 44))
SENTINEL = 0x5A
NAN = float("nan")


def _lib():
    from simpb_amd import _lib as L
    return L


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def table(live):
    """The live-image table of `live`; the entries behind L name the highest dead image (they must not be read)."""
    dead = [i for i in range(N) if i not in live]
    t = torch.full((1 + N,), dead[-1] if dead else 0, dtype=torch.int32)
    t[0] = len(live)
    t[1:1 + len(live)] = torch.tensor(sorted(live), dtype=torch.int32)
    return t.cuda()


def sentinel(shape, dtype):
    """A device tensor of `shape` whose every byte is SENTINEL (finite as f16 and as f32)."""
    nbytes = torch.empty((), dtype=dtype).element_size()
    for d in shape:
        nbytes *= d
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)


def rand(shape, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half().cuda()


def poisoned(t, live):
    """t [N, ...] with every dead image's rows NaN."""
    out = t.clone()
    for i in range(N):
        if i not in live:
            out[i] = NAN
    return out


def expect(ref, live):
    """The sentinel buffer with the live images' rows of `ref` (itself launched into a sentinel buffer) put in."""
    out = sentinel(ref.shape, ref.dtype)
    for i in live:
        out[i] = ref[i]
    return out


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def check(ok, what):
    assert ok == 0, (what, ok, _lib().lib().simpb_last_error())


# ------------------------------------------------------------------------------------------------------------------ conv1x1
def conv1x1(x, w, b, res, stride, up2, in_bias, variant, live):
    """x [N, H, W, Cin] -> y [N, ho, wo, Cout] launched into a sentinel buffer; live None: the entry point without the suffix."""
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    y = sentinel((n, ho, wo, cout), torch.float16)
    args = (_p(y), _p(x), _p(w), _p(b), _p(res), n, h, wd, cin, cout, stride, 1, 1 if up2 else 0, _p(in_bias), variant, _stream())
    lib = _lib().lib()
    if live is None:
        check(lib.simpb_conv1x1_nhwc_f16(*args), "conv1x1")
    else:
        check(lib.simpb_conv1x1_nhwc_f16_live(*args, _p(live)), "conv1x1 live")
    return y


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
def test_conv1x1_live_forms(variant):
    seed = 100 * variant
    for (h, wd) in MAPS:
        for cin, cout in ((64, 128), (128, 64)):
            w, b = rand((cout, cin), 0.08, seed + 1), rand((cout,), 0.5, seed + 2)
            x = rand((N, h, wd, cin), 0.7, seed + 3)
            for stride in (1, 2):
                ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
                kinds = ["plain", "residual"] + (["up2"] if ho % 2 == 0 and wo % 2 == 0 else []) + (["in_bias"] if variant == 1 else [])
                for kind in kinds:
                    res = (rand((N, ho, wo, cout), 0.5, seed + 4) if kind == "residual" else
                           rand((N, ho // 2, wo // 2, cout), 0.5, seed + 5) if kind == "up2" else None)
                    ib = rand((cin,), 0.3, seed + 6) if kind == "in_bias" else None
                    ref = conv1x1(x, w, b, res, stride, kind == "up2", ib, variant, None)
                    assert bool(torch.isfinite(ref.float()).all())
                    for live in LIVE_SETS:
                        got = conv1x1(poisoned(x, live), w, b, poisoned(res, live) if res is not None else None, stride,
                                      kind == "up2", ib, variant, table(live))
                        assert same_bytes(got, expect(ref, live)), (variant, h, wd, cin, cout, stride, kind, live)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ conv3x3
def conv3x3(x, w, b, stride, variant, dest, live):
    """dest "y": -> y [N, ho, wo, Cout]; "tok": -> (f32 rows, f16 rows) [N, per_cam, Cout] with this level at row 3 of a
    camera's block; "tok16": -> the f16 rows alone. All launched into sentinel buffers."""
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    per_cam, start = ho * wo + 7, 3
    y = sentinel((n, ho, wo, cout), torch.float16) if dest == "y" else None
    t32 = sentinel((n, per_cam, cout), torch.float32) if dest == "tok" else None
    t16 = sentinel((n, per_cam, cout), torch.float16) if dest != "y" else None
    args = (_p(y), _p(t32), _p(t16), per_cam if dest != "y" else 0, start if dest != "y" else 0, _p(x), _p(w), _p(b), n, h, wd, cin,
            cout, stride, 1 if dest == "y" else 0, variant, _stream())
    lib = _lib().lib()
    if live is None:
        check(lib.simpb_conv3x3_nhwc_f16(*args), "conv3x3")
    else:
        check(lib.simpb_conv3x3_nhwc_f16_live(*args, _p(live)), "conv3x3 live")
    return [t for t in (y, t32, t16) if t is not None]


@pytest.mark.parametrize("variant", range(1, 14))
def test_conv3x3_live_forms(variant):
    seed = 1000 + 100 * variant
    strides = (1,) if variant >= 12 else (1, 2)   # the resident forms are stride 1
    for (h, wd) in MAPS:
        for cin, cout in ((64, 64), (128, 128), (64, 128)):
            w, b = rand((cout, 3, 3, cin), 0.04, seed + 1), rand((cout,), 0.5, seed + 2)
            x = rand((N, h, wd, cin), 0.7, seed + 3)
            for stride in strides:
                for dest in ("y", "tok", "tok16"):
                    refs = conv3x3(x, w, b, stride, variant, dest, None)
                    assert all(bool(torch.isfinite(r.float()).all()) for r in refs)
                    for live in LIVE_SETS:
                        gots = conv3x3(poisoned(x, live), w, b, stride, variant, dest, table(live))
                        for got, ref in zip(gots, refs):
                            assert same_bytes(got, expect(ref, live)), (variant, h, wd, cin, cout, stride, dest, live, got.dtype)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ group launch
LEVELS = ((16, 44), (8, 22), (4, 11), (2, 6))


def group(xs, ws, bs_, variants, f32_rows, live):
    cin, cout = xs[0].shape[-1], ws[0].shape[0]
    k = len(xs)
    sizes = [h * w for h, w in LEVELS]
    per_cam = sum(sizes) + 5
    starts = [2 + sum(sizes[:i]) for i in range(k)]
    t32 = sentinel((N, per_cam, cout), torch.float32) if f32_rows else None
    t16 = sentinel((N, per_cam, cout), torch.float16)
    arr_p, arr_i = ctypes.c_void_p * k, ctypes.c_int * k
    args = (k, _p(t32), _p(t16), per_cam, arr_i(*starts), arr_p(*[x.data_ptr() for x in xs]), arr_p(*[w.data_ptr() for w in ws]),
            arr_p(*[b.data_ptr() for b in bs_]), N, arr_i(*[h for h, _ in LEVELS]), arr_i(*[w for _, w in LEVELS]), cin, cout, 0,
            arr_i(*variants), _stream())
    lib = _lib().lib()
    if live is None:
        check(lib.simpb_conv3x3_group_tokens_forms_f16(*args), "group")
    else:
        check(lib.simpb_conv3x3_group_tokens_forms_f16_live(*args, _p(live)), "group live")
    return [t for t in (t32, t16) if t is not None]


@pytest.mark.parametrize("forms", [(8, 8, 8, 8), (13, 13, 13, 13), (13, 8, 13, 8)], ids=["staged", "resident", "mixed"])
def test_group_token_launch_live_forms(forms):
    seed = 5000 + sum(forms)
    for cin, cout in ((128, 128), (64, 128)):
        xs = [rand((N, h, w, cin), 0.7, seed + j) for j, (h, w) in enumerate(LEVELS)]
        ws = [rand((cout, 3, 3, cin), 0.04, seed + 10 + j) for j in range(4)]
        bs_ = [rand((cout,), 0.5, seed + 20 + j) for j in range(4)]
        for f32_rows in (True, False):
            refs = group(xs, ws, bs_, forms, f32_rows, None)
            for live in LIVE_SETS:
                gots = group([poisoned(x, live) for x in xs], ws, bs_, forms, f32_rows, table(live))
                for got, ref in zip(gots, refs):
                    assert same_bytes(got, expect(ref, live)), (forms, cin, cout, f32_rows, live, got.dtype)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------------- stem
def test_stem_live_form():
    from simpb_amd.plugin import ops
    h, wd = 64, 176
    x4 = rand((N, h, wd, 4), 1.0, 7001)
    x4[..., 3] = 0
    weight, bias = rand((64, 3, 7, 7), 0.05, 7002), rand((64,), 0.3, 7003)
    pack = ops._stem_weight_packed(weight)
    lib = _lib().lib()

    def run(x, live):
        out = sentinel((N, 16, 44, 64), torch.float16)
        args = (_p(out), _p(x), _p(pack), _p(bias), N, h, wd, 64, _stream())
        if live is None:
            check(lib.simpb_stem_conv7x7_pool_f16(*args), "stem")
        else:
            check(lib.simpb_stem_conv7x7_pool_f16_live(*args, _p(live)), "stem live")
        return out

    ref = run(x4, None)
    assert bool(torch.isfinite(ref.float()).all())
    for live in LIVE_SETS:
        assert same_bytes(run(poisoned(x4, live), table(live)), expect(ref, live)), live
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ the operator layer
def test_operators_hand_the_table_down():
    """ops.conv1x1_nhwc / conv3x3_nhwc / stem_conv_pool_nhwc4 with live= : the live images' rows of what they return equal
    the full call's (their dead rows are whatever the allocation held), and a table of another size is refused."""
    from simpb_amd.plugin import ops
    live = (1, 3)
    t = table(live)
    x = rand((N, 8, 22, 64), 0.7, 9001).permute(0, 3, 1, 2)           # channels_last [N, C, H, W]
    w1, w3, b = rand((128, 64, 1, 1), 0.08, 9002), rand((128, 64, 3, 3), 0.04, 9003).contiguous(memory_format=torch.channels_last), rand((128,), 0.5, 9004)
    xp = poisoned(x, live)
    for full, part in ((ops.conv1x1_nhwc(x, w1, b), ops.conv1x1_nhwc(xp, w1, b, live=t)),
                       (ops.conv3x3_nhwc(x, w3, b), ops.conv3x3_nhwc(xp, w3, b, live=t))):
        for i in live:
            assert torch.equal(full[i], part[i]), i
    x4 = rand((N, 64, 176, 4), 1.0, 9005)
    weight, bias = rand((64, 3, 7, 7), 0.05, 9006), rand((64,), 0.3, 9007)
    full, part = ops.stem_conv_pool_nhwc4(x4, weight, bias), ops.stem_conv_pool_nhwc4(poisoned(x4, live), weight, bias, live=t)
    for i in live:
        assert torch.equal(full[i], part[i]), i
    for bad in (t[:-1].contiguous(), t.long(), t.cpu()):
        with pytest.raises(ValueError, match="live"):
            ops.conv1x1_nhwc(x, w1, b, live=bad)
