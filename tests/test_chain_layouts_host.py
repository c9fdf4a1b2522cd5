"""Host side of the MLP-chain kernels (plugin/fused.py), without a GPU: the three weight layouts element by element, the
cache of the repacked copies, and which form and which layout a launch takes."""
import itertools

import pytest
import torch
import torch.nn as nn

from simpb_amd.plugin import fused, routes

SHAPES = [(7, 12), (33, 64), (100, 96), (255, 256)]   # (out, in)
# weights_transposed -> K divisor of the packed layout (None: nn.Linear's own layout for every layer), as csrc/mlp_chain.hip
# reads them: 16-row kernel in place, VALU kernel transposed, 4-row kernel k4-packed, 32-row kernel fragment-packed
DIVISOR = {0: None, 1: 1, 2: 4, 3: 32}


def _weight(n, k):
    return (torch.arange(n * k, dtype=torch.float32).reshape(n, k) + 1) / 8     # distinct, exact in fp32


@pytest.mark.parametrize("n,k", SHAPES)
def test_k4_packed_layout(n, k):
    w = _weight(n, k)
    wp = fused.pack_k4(w)
    assert wp.shape == (k // 4, n, 4) and wp.is_contiguous() and wp.dtype == torch.float32
    kk, nn_ = torch.meshgrid(torch.arange(k), torch.arange(n), indexing="ij")
    assert torch.equal(wp[kk // 4, nn_, kk % 4], w.t())


@pytest.mark.parametrize("n,k", [s for s in SHAPES if s[1] % 32 == 0])
def test_fragment_packed_layout(n, k):
    w = _weight(n, k)
    wq = fused.pack_fragments(w)
    tiles = -(-n // 32)
    assert wq.numel() == tiles * 32 * k and wq.is_contiguous() and wq.dtype == torch.float32
    wq = wq.reshape(tiles, k // 32, 4, 64, 4)     # the kernel's view: [tile][chunk][q][lane][4]
    t, c, q, h, r, e = torch.meshgrid(torch.arange(tiles), torch.arange(k // 32), torch.arange(4), torch.arange(2),
                                      torch.arange(32), torch.arange(4), indexing="ij")
    row, col = 32 * t + r, 32 * c + 16 * h + 4 * q + e
    full = torch.zeros(tiles * 32, k)
    full[:n] = w
    got = wq[t, c, q, 32 * h + r, e]
    assert torch.equal(got, full[row, col])
    assert bool((got[row >= n] == 0).all()) and bool((got[row < n] != 0).all())


@pytest.mark.parametrize("n,k", SHAPES)
def test_transposed_layout(n, k):
    w = _weight(n, k)
    wt = fused.pack_transposed(w)
    assert wt.is_contiguous() and wt.dtype == torch.float32 and torch.equal(wt, w.t())


def _filled(plan, form):
    chain, keep = fused._Chain(), []
    plan.fill(chain, keep, form)
    return chain, keep


def test_packed_copy_follows_the_parameter():
    """The same object while nothing changed; refreshed after an in-place update and after the parameter is replaced."""
    lin = nn.Linear(64, 33)
    plan = fused.ChainPlan(nn.Sequential(lin))
    for form, pack in ((1, fused.pack_transposed), (2, fused.pack_k4), (3, fused.pack_fragments)):
        chain, keep = _filled(plan, form)
        first = keep[0]
        assert chain.ops[0].w == first.data_ptr() and torch.equal(first, pack(lin.weight.detach()))
        assert _filled(plan, form)[1][0] is first
        with torch.no_grad():
            lin.weight.mul_(2)
        second = _filled(plan, form)[1][0]
        assert second is not first and torch.equal(second, pack(lin.weight.detach()))
        assert _filled(plan, form)[1][0] is second
        lin.weight = nn.Parameter(torch.randn(33, 64))
        third = _filled(plan, form)[1][0]
        assert third is not second and torch.equal(third, pack(lin.weight.detach()))
        assert _filled(plan, form)[1][0] is third


def test_form_and_layout_of_every_route():
    """launch_form returns what run_chains passed before there was such a function, for every combination of the routes, the
    row counts round WIDE_ROWS and sine / no sine; fill takes the packed copy exactly when the form's divisor divides in_dim."""
    widths = [3, 12, 32, 64, 100, 96, 256, 255]
    mods = []
    for k, d in zip(widths, widths[1:] + [5]):
        mods += [nn.Linear(k, d), nn.ReLU()]
    seq = nn.Sequential(*mods)
    plan = fused.ChainPlan(seq)
    lins = [m for m in seq if isinstance(m, nn.Linear)]
    seen = set()
    for rows4, transposed, sine in itertools.product((False, True), repeat=3):
        for rows in (1, fused.WIDE_ROWS - 1, fused.WIDE_ROWS):
            with routes.override(chain_rows4=rows4, chain_transposed=transposed):
                wide = rows4 and rows >= fused.WIDE_ROWS and not sine
                want = 3 if wide else 2 if rows4 else (1 if transposed else 0)
                form = fused.launch_form(rows, sine)
                assert form == want, (rows4, transposed, sine, rows)
                assert (form in fused.LEAD_NORM) == (want in (2, 3))
                chain, keep = _filled(plan, form)
            seen.add(form)
            kept = {t.data_ptr() for t in keep}
            assert chain.n_ops == len(lins)
            for j, lin in enumerate(lins):
                packed = DIVISOR[form] is not None and lin.in_features % DIVISOR[form] == 0
                assert (chain.ops[j].w in kept) == packed, (form, lin.in_features)
                assert (chain.ops[j].w == lin.weight.data_ptr()) == (not packed), (form, lin.in_features)
                assert chain.ops[j].b == lin.bias.data_ptr()
    assert seen == {0, 1, 2, 3}


def test_launch_form_reads_wide_rows_at_call_time():
    keep = fused.WIDE_ROWS
    try:
        fused.WIDE_ROWS = 1
        assert fused.launch_form(1, False) == 3 and fused.launch_form(1, True) == 2
        fused.WIDE_ROWS = 1 << 30
        assert fused.launch_form(1 << 20, False) == 2
    finally:
        fused.WIDE_ROWS = keep
