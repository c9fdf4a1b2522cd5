"""CPU: one migration through the head on its torch path -- the PyTorch statement of InstanceBank.export_stream /
import_stream (the non-fused route, state in ordinary tensors) carrying a stream from one head to another, against the
stay-at-home run. The frame runners need a device for their read-back, so the two "runners" here are two copies of the head
driven frame by frame, as tests/test_lean_host.py drives one, with that file's torch stand-ins for the operators that exist
as HIP kernels only; what is under test is that NOTHING but the record and the previous frame's metas has to travel."""
import copy

import torch

from simpb_amd import synth
from tests.helpers import build_product_head
from tests.test_lean_host import SPEC, _stand_ins  # noqa: F401  (autouse fixture: the stand-ins apply to this file too)

FRAMES, MOVE = 6, 3
KEYS = ("prediction", "classification", "quality", "prediction2d", "classification2d")


def _frame(f):
    from oracle import simpb_ref as R
    return R.feature_maps_format(synth.feature_maps_nchw(1, f, SPEC["image_wh"])), synth.frame_metas(1, f, SPEC["image_wh"])


def test_a_stream_moved_between_two_heads_goes_on_as_if_it_had_stayed():
    """Head X decodes the stream's frames 0-5. Head Y decodes somebody else's frames (other maps, a clock 40 s away) for three
    steps, then takes X's record and the metas of X's last frame and decodes frames 3-5: every output list and the bank's
    float rows equal X's exactly; ids agree under one relabelling, and every id Y issues after the move lies above the
    record's -- X's counter was put 10 000 above Y's, so this fails without the floor on prev_id."""
    from simpb_amd.plugin.instance_bank import record_header
    pristine = build_product_head(SPEC, "cpu")
    x, y = copy.deepcopy(pristine), copy.deepcopy(pristine)
    home = []
    with torch.no_grad():
        for f in range(FRAMES):
            maps, metas = _frame(f)
            out = x(maps, metas)
            bank = x.instance_bank
            if f == 0:
                bank.prev_id = bank.prev_id + 10_000
                bank.instance_id = torch.where(bank.instance_id >= 0, bank.instance_id + 10_000, bank.instance_id)
            if f == MOVE - 1:
                record, last_metas = bank.export_stream(0), bank.metas
            home.append((out, {k: getattr(bank, k).clone() for k in ("cached_feature", "cached_anchor", "confidence", "instance_id")}))
        carried = record_header(record)
        in_record = set(v for v in home[MOVE - 1][1]["instance_id"].flatten().tolist() if v >= 0)
        assert carried["largest_id"] >= 10_000 and not record.is_cuda
        for f in range(MOVE):
            maps, metas = _frame(f + 10)
            metas["timestamp"] = metas["timestamp"] + 40.0
            y(maps, metas)
        yb = y.instance_bank
        assert int(yb.prev_id) < 10_000
        yb.import_stream(0, record)
        yb.metas = last_metas
        assert int(yb.prev_id) == carried["largest_id"] + 1
        fwd, back = {}, {}
        for f in range(MOVE, FRAMES):
            maps, metas = _frame(f)
            got, (want, want_bank) = y(maps, metas), home[f]
            for k in KEYS:
                for li, (a, b) in enumerate(zip(got[k], want[k])):
                    assert (a is None and b is None) or torch.equal(a, b), (f, k, li)
            for k in ("cached_feature", "cached_anchor", "confidence"):
                assert torch.equal(getattr(yb, k), want_bank[k]), (f, k)
            for a, b in ((got["instance_id"], want["instance_id"]), (yb.instance_id, want_bank["instance_id"])):
                for u, v in zip(a.flatten().tolist(), b.flatten().tolist()):
                    assert (u < 0) == (v < 0)
                    if u >= 0:
                        assert fwd.setdefault(u, v) == v and back.setdefault(v, u) == u, (f, u, v)
            ids = got["instance_id"].flatten()
            fresh = [v for v in ids.tolist() if v >= 0 and v not in in_record]
            assert all(v > carried["largest_id"] for v in fresh), (f, fresh[:5])
            assert all(fwd[v] == v for v in ids.tolist() if v in in_record)   # a carried id is still the same track's
        assert any(u in in_record for u in fwd) and any(u not in in_record for u in fwd)
