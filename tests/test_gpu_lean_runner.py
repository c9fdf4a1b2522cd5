"""GPU: a runner's replayed frames with the three lean routes on (routes.lean_tokens, routes.lean_refine2d, routes.lean_glue:
f16 token rows alone, no refinement head whose outputs only training reads, the projection rows read in place) against the same runner with them off -- the parent behaviour in
the same tree. Small real detector (tests/test_gpu_camera_dropout.py: fp16 ResNet50 + FPN, raw u8 frames 800 x 300 ->
352 x 128, capacity 256), two runners from deep copies of one model, 5 frames each so that both replay: frame 0 is cold,
frames 2 and 3 run the eager decoder on the tokens of a CAPTURED backbone (f16 rows alone in the lean runner), frame 4 is
decoded by a replayed graph. Frame by frame the 3D and 2D records, the overflow words and the bank's static state are
bit-equal; the lean runner's graphs hold no fp32 token buffer."""
import copy

import pytest
import torch

from simpb_amd import synth
from tests.test_gpu_camera_dropout import SRC, WH, _pristine

pytestmark = pytest.mark.gpu

FRAMES = 5
LEAN_OFF = dict(lean_tokens=False, lean_refine2d=False, lean_glue=False)


def _metas(bs, f):
    metas = synth.frame_metas(bs, f, WH)
    for m in metas["img_metas"]:
        m["aug_config"] = dict(resize=0.44, crop=(0, 4, 352, 132))
    return metas


def _bytes(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu()


def _pool_bytes(r):
    """(bytes reserved, bytes held by live blocks) of the private pools of this runner's graphs."""
    graphs = [g for g in list(r.bb_graph) + list(r.head_graph) + list(getattr(r, "pre_graph", [])) if g is not None]
    pools = {tuple(g.pool()) for g in graphs}
    reserved = held = 0
    for seg in torch.cuda.memory_snapshot():
        if tuple(seg.get("segment_pool_id", (0, 0))) in pools:
            reserved += seg["total_size"]
            held += sum(b["size"] for b in seg["blocks"] if b["state"] != "inactive")
    return reserved, held


def _run(kind, bs, lean):
    """FRAMES frames through one runner -> (runner, per step: records of the frame returned + overflow words + bank state)."""
    from simpb_amd import runner as RN
    from simpb_amd.plugin import routes
    cls = dict(split=RN.SplitPipelinedRunner, pipe=RN.PipelinedRunner)[kind]
    seen = []
    with routes.override(**({} if lean else LEAN_OFF)):
        r = cls(copy.deepcopy(_pristine()), bs, (WH[1], WH[0]), capacity=256, device=torch.device("cuda"), use_graph=True,
                raw_input=SRC, independent_streams=bs > 1)
        for f in range(FRAMES + 1):
            res = r.step(synth.raw_frames(bs, f % 3, SRC).cuda(), _metas(bs, f)) if f < FRAMES else r.flush()
            torch.cuda.synchronize()   # decoder(f) has run: the state below is the state after frame f
            state = {k: _bytes(v) for k, v in r.head.instance_bank._static.items() if torch.is_tensor(v)}
            words = [_bytes(r.flags)] + ([_bytes(r.hb), _bytes(r.sticky)] if kind == "split" else [])
            rec = (_bytes(r.last_rec3d), _bytes(r.last_rec2d)) if res is not None else None
            seen.append((rec, words, state))
        assert r.stats["replay"] >= 1 and r.stats["overflow"] == 0, r.stats
        assert all(g is not None for g in r.bb_graph) and any(g is not None for g in r.head_graph)
    return r, seen


@pytest.mark.parametrize("kind,bs", [("split", 1), ("pipe", 2)])
def test_lean_replayed_frames_equal_the_full_ones_bit_for_bit(kind, bs):
    full, a = _run(kind, bs, lean=False)
    lean, b = _run(kind, bs, lean=True)
    assert full.stats == lean.stats, (full.stats, lean.stats)
    for f, ((rec_a, words_a, state_a), (rec_b, words_b, state_b)) in enumerate(zip(a, b)):
        assert (rec_a is None) == (rec_b is None), f
        if rec_a is not None:
            assert torch.equal(rec_a[0], rec_b[0]), (kind, f, "rec3d")
            assert torch.equal(rec_a[1], rec_b[1]), (kind, f, "rec2d")
        for i, (x, y) in enumerate(zip(words_a, words_b)):
            assert torch.equal(x, y), (kind, f, "overflow word", i)
        assert state_a and set(state_a) == set(state_b)
        for k in state_a:
            assert torch.equal(state_a[k], state_b[k]), (kind, f, "bank", k)
    assert any(rec is not None and bool(rec[0].any()) for rec, _, _ in b)   # (the records are not empty buffers)

    # the lean runner's graphs hold no fp32 token buffer. Each slot's backbone graph keeps its token rows alive as its output:
    # fp32 + f16 rows in the full runner, f16 rows alone in the lean one. Checked by size on the bytes the graphs' pools hold
    # in live blocks (exact), not on the bytes they reserve: the allocator reserves whole segments and rounds them (2 MiB
    # steps; 20 MiB for blocks of 1-10 MiB), so the reserved figure moves by about, not exactly, what left the pool. Measured
    # (profiles/lean_frames.md): split bs 1 reserves 184.5 / 140.5 MB, 44.0 MB less for 45.96 MB of fp32 rows, while the live
    # blocks shrink by 46.1 MB; pipelined bs 2 reserves 92.3 MB less for 91.9 MB. The reserved bytes may not grow.
    tokens = full.fm[0][0]
    assert tokens.dtype == torch.float32 and getattr(tokens, "simpb_f16", None) is not None
    assert all(fm[0].dtype == torch.float16 for fm in lean.fm)
    fp32_rows = tokens.numel() * 4 * 2          # two feature slots
    (res_full, held_full), (res_lean, held_lean) = _pool_bytes(full), _pool_bytes(lean)
    print(f"{kind} bs {bs}: graph pools reserve {res_full} / {res_lean} bytes (full / lean), hold {held_full} / {held_lean}; "
          f"fp32 rows of two slots {fp32_rows}")
    assert res_full > 0 and res_lean <= res_full
    assert held_full - held_lean >= fp32_rows, (held_full, held_lean, fp32_rows)
