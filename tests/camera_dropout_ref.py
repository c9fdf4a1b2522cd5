"""The yardstick of camera dropout: "camera c is missing" means the frame is decoded exactly as the reference decodes it when
given the REMAINING cameras only. The committed oracle (oracle/simpb_ref.py) takes the number of cameras from the shapes
of its inputs everywhere except the default num_cams=6 of `dfa_weights`, which `bind_cameras` re-binds at run time (through
the test's monkeypatch, so the module is as it was after the test). No GPU, no product code."""
import functools

import torch

from oracle import simpb_ref as R

DFA_WEIGHTS = R.dfa_weights   # the function as committed (a bound partial is never bound again)
ALL = (0, 1, 2, 3, 4, 5)


def bind_cameras(monkeypatch, kept):
    monkeypatch.setattr(R, "dfa_weights", functools.partial(DFA_WEIGHTS, num_cams=len(kept)))


def subset_frame(maps, metas, kept, sample=None):
    """(feature maps in the oracle's format, metas) of the kept cameras; sample=b: that sample alone, as a batch of one."""
    kept = list(kept)
    rows = slice(None) if sample is None else slice(sample, sample + 1)
    fm = R.feature_maps_format([m[rows][:, kept] for m in maps])
    out = dict(metas, projection_mat=metas["projection_mat"][rows][:, kept], image_wh=metas["image_wh"][rows][:, kept],
               timestamp=metas["timestamp"][rows])
    if sample is not None:
        out["img_metas"] = [metas["img_metas"][sample]]
    return fm, out


def oracle_frame(monkeypatch, oracle, maps, metas, kept, sample=None):
    """One frame of `oracle` (its bank carries over between calls, whatever the camera sets) on the kept cameras. Returns the
    output dict and the frame's two top-k margins on the oracle's own numbers, the smallest over the batch: `update` -- the
    cut of InstanceBank.update (best A - T current instances by the first layer's max-class logit), None on a frame without
    history -- and `cache`, the cut of InstanceBank.cache (best T by confidence), which decides what the NEXT frame sees."""
    bind_cameras(monkeypatch, kept)
    fm, sub = subset_frame(maps, metas, kept, sample)
    warm = oracle.bank.cached_feature is not None
    want = oracle.forward(fm, sub)
    bank = oracle.bank
    cuts = dict(update=None, cache=None)
    if warm and bool(bank.mask.all()):
        v = torch.sort(want["classification"][0].max(dim=-1).values, dim=1, descending=True).values
        k = bank.num_anchor - bank.num_temp
        cuts["update"] = float((v[:, k - 1] - v[:, k]).min())
    c = torch.sort(bank.temp_confidence, dim=1, descending=True).values
    cuts["cache"] = float((c[:, bank.num_temp - 1] - c[:, bank.num_temp]).min())
    return want, cuts


def mask_rows(kept_per_sample, num_cams=6):
    """[[bool] * num_cams per sample] from the kept camera indices of each sample."""
    return [[c in kept for c in range(num_cams)] for kept in kept_per_sample]
