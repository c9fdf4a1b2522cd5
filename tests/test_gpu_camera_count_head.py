"""GPU: the decoder at 1, 5 and 8 cameras against the oracle, per stream.

The recipe of tests/test_gpu_head.py::test_batch_of_independent_streams_vs_oracle_per_stream on the small golden spec (image
176 x 64, 48 anchors, 32 temporal, 20 outputs): bs 2 independent streams through FrameRunner(use_graph=False), three frames,
tokens that are f16 numbers with their f16 copy attached, against OracleHead at bs = 1 per stream (its one default of six
cameras re-bound by tests/camera_dropout_ref.py::bind_cameras). On warm frames the oracle of a stream starts from the bank
state the batch held for that stream. Cold frame: every head output position by position at 1e-3 and the group table exact.
Warm frames: as row sets at 1e-3, both ways. Final detections via helpers.compare_result.

There is NO tie allowance: tests/test_camera_count_host.py shows that on these seeds the oracle alone has no ranking cut and
no projected centre within 1e-4 of flipping, so a row without a partner fails the test. A spy asserts that every 3D
aggregation of the frame was the one launch (csrc/deform_agg_fused.hip) and the three-launch route never ran."""
import numpy as np
import pytest
import torch

from tests import camera_count_cases as K
from tests import camera_dropout_ref as C
from tests.helpers import compare_result
from tests.test_gpu_head import _oracle_result_as_golden, _Served

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", K.HEAD_CAMS)
def test_head_at_n_cameras_vs_oracle_per_stream(n, monkeypatch):
    from oracle import simpb_ref as R
    from simpb_amd.plugin import blocks, ops
    from simpb_amd.runner import FrameRunner
    spec = K.head_spec()
    wh, bs = spec["image_wh"], K.HEAD_BS
    head = K.build_head(spec, n, "cuda")
    params = {k: v.detach().cpu() for k, v in head.state_dict().items()}
    C.bind_cameras(monkeypatch, range(n))
    calls = dict(one=0, three=0)

    def spy_fused(*a, **kw):
        calls["one"] += 1
        return ops.dfa_fused(*a, **kw)

    def spy_three(*a, **kw):
        calls["three"] += 1
        return ops.deformable_aggregation_function(*a, **kw)

    monkeypatch.setattr(blocks, "dfa_fused", spy_fused)
    monkeypatch.setattr(blocks, "DAF", spy_three)
    served = _Served(head)
    runner = FrameRunner(served, bs, (wh[1], wh[0]), capacity=K.HEAD_CAPACITY, device=torch.device("cuda"), use_graph=False,
                         independent_streams=True)
    captured = {}
    head.register_forward_hook(lambda m, i, o: captured.update(outs=o))
    bank = head.instance_bank
    deformable = head.operation_order.count("deformable")
    prev_metas = None
    with torch.no_grad():
        for f in range(K.HEAD_FRAMES):
            maps, metas = K.frame_inputs(spec, n, f)
            fm_cpu = R.feature_maps_format(maps)
            fm = ops.feature_maps_format([x.cuda() for x in maps])
            fm[0].simpb_f16 = fm[0].half()
            served.maps = fm
            torch.cuda.synchronize()
            state = {k: v.clone().cpu() for k, v in bank._static.items()}
            got = runner.step(runner.img, metas)
            outs = captured["outs"]
            assert runner.stats["overflow"] == 0
            assert calls == dict(one=deformable * (f + 1), three=0), calls
            gs = outs["alloc_list"][-1].group_start.cpu().numpy()
            for b in range(bs):
                one = K.one_stream(metas, b)
                oracle = R.OracleHead(params, head.operation_order, spec["num_anchor"], spec["num_temp"], spec["num_output"])
                if f > 0:   # the state the batch held for this stream in front of the frame
                    ob = oracle.bank
                    ob.cached_feature, ob.cached_anchor = state["cached_feature"][b:b + 1].clone(), state["cached_anchor"][b:b + 1].clone()
                    ob.confidence, ob.instance_id = state["confidence"][b:b + 1].clone(), state["instance_id"][b:b + 1].clone()
                    ob.prev_id = int(state["prev_id"])
                    ob.metas = dict(timestamp=prev_metas["timestamp"][b:b + 1], img_metas=[prev_metas["img_metas"][b]])
                want = oracle.forward([fm_cpu[0][b:b + 1], fm_cpu[1], fm_cpu[2]], one)
                margins = K.margins(want, oracle, one, spec, f > 0)
                lo, hi = int(gs[b * n]), int(gs[(b + 1) * n])
                n2 = want["prediction2d"][-1].shape[1]
                starts = np.asarray([g[0] for g in want["ref_query_groups_list"][-1]] + [n2])
                print(f"FIG N{n} frame {f} stream {b} slots={hi - lo} (oracle {n2}) groups={np.diff(starts).tolist()} "
                      f"oracle margins={ {k: f'{v:.1e}' for k, v in margins.items()} }")
                assert hi - lo == n2, (f, b, hi - lo, n2)
                assert np.array_equal(gs[b * n:b * n + n + 1] - lo, starts), (f, b)     # the group table, exact
                worst = 0.0
                for k in ("prediction", "classification", "quality", "prediction2d", "classification2d"):
                    for li, (a, w_) in enumerate(zip(outs[k], want[k])):
                        if w_ is None:
                            assert a is None
                            continue
                        if k.endswith("2d"):
                            gl = outs["alloc_list"][li].group_start.cpu().numpy()
                            a = a[0, int(gl[b * n]):int(gl[(b + 1) * n])]
                            assert a.shape[0] == w_.shape[1], (f, b, k, li)
                        else:
                            a = a[b]
                        if f == 0:
                            err = (a.cpu() - w_[0]).abs().max(dim=-1).values
                        else:   # as row sets: every row needs a partner, both ways
                            d = torch.cdist(a.cpu().double(), w_[0].double(), p=float("inf"))
                            err = torch.maximum(d.min(dim=1).values, d.min(dim=0).values)
                        worst = max(worst, float(err.max()))
                        assert float(err.max()) <= 1e-3, (n, f, b, k, li, float(err.max()), int((err > 1e-3).sum()))
                print(f"FIG N{n} frame {f} stream {b} worst row error={worst:.2e}")
                compare_result(got[b]["img_bbox"], _oracle_result_as_golden(oracle.post_process(want, one)[0], "w."), "w.")
            prev_metas = metas
