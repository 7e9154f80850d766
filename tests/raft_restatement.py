"""Test-side helper (not a test): a pure-torch restatement of the RAFT baseline decoders, composed
from the oracle's hot-path functions plus RAFT's convex upsampling, and what the RAFT tests share
(the fixture, the reference-style configs, the seeded weights with the fixture's gain).

The decoder loop follows ``models/decoder/raft_decoder.py:434-457`` (``RAFTDecoder.forward``) and
``models/decoder/raft_decoder_mask.py:179-208`` (``RAFTDecoderMask.forward``); the upsampling
``raft_decoder.py:381-416`` / ``raft_decoder_mask.py:141-160``.  It is pinned to the reference by
``tests/test_raft_host.py`` (the fixture ``tests/golden/make_golden_raft.py`` writes from the
reference's own modules).
"""
import os
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from oracle import scflow_oracle as orc
from scflow_amd import synthetic
from tests.helpers import GOLDEN

EPE_TOL = 1e-3  # px: the project's gate (tests/test_gpu_decoder.py:17)


@lru_cache(maxsize=None)
def raft_golden():
    out = {}
    for name in ("golden_raft_b2_s256_it4.npz", "golden_raft_b2_s256_it4_upflow.npz"):
        with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    return out


def raft_decoder_cfg(iters=4, **over):
    """The decoder block of the reference's configs/refine_models/raft.py:40-48, without `type`."""
    cfg = dict(net_type="Basic", num_levels=4, radius=4, iters=iters,
               corr_lookup_cfg=dict(align_corners=True), gru_type="SeqConv",
               act_cfg=dict(type="ReLU"))
    cfg.update(over)
    return cfg


def reference_state_shapes(tag):
    """(key, shape) of the reference module's state dict: tag 'mask' (RAFTDecoderMask) / 'plain'."""
    g = raft_golden()
    return [(str(k), tuple(int(s) for s in str(v).split(",") if s))
            for k, v in zip(g[f"state_keys_{tag}"], g[f"state_shapes_{tag}"])]


def apply_gain_(sd_or_module, gain):
    """The fixture's gain on the mask predictor's weights (see make_golden_raft.py)."""
    if isinstance(sd_or_module, dict):
        sd_or_module["mask_pred.predict_layer.weight"] = \
            sd_or_module["mask_pred.predict_layer.weight"] * gain
    else:
        with torch.no_grad():
            sd_or_module.mask_pred.predict_layer.weight.mul_(gain)
    return sd_or_module


def raft_state_dict(tag="mask", seed=0, gain=None, dtype=torch.float32):
    """What a reference module filled with ``fill_module_(seed)`` and the gain holds."""
    gain = float(raft_golden()["gain"]) if gain is None else gain
    vals = synthetic.make_state_dict(reference_state_shapes(tag), seed=seed)
    sd = {k: torch.from_numpy(v).to(dtype) for k, v in vals.items()}
    return apply_gain_(sd, gain)


def build_raft_decoder(kind="RAFTDecoderMask", iters=4, seed=0, gain=None, **over):
    from scflow_amd import MODELS
    gain = float(raft_golden()["gain"]) if gain is None else gain
    dec = MODELS.build(dict(type=kind, **raft_decoder_cfg(iters, **over)))
    synthetic.fill_module_(dec, seed=seed)
    return apply_gain_(dec, gain).eval()


def raft_inputs(B, S, seed, g=None, dtype=torch.float32):
    """feat1 (rendered), feat2 (real), zero flow at the feature resolution, h, cxt; with a fixture
    dict the regenerated arrays are checked against its checksums."""
    raw = synthetic.make_decoder_inputs(B, S, seed=seed)
    if g is not None:
        for k in ("feat_render", "feat_real", "h_feat", "cxt_feat"):
            got = np.array([raw[k].astype(np.float64).sum(), np.abs(raw[k]).astype(np.float64).sum()])
            np.testing.assert_allclose(got, g[f"sum_{k}"], rtol=1e-9, atol=1e-6)
    t = {k: torch.from_numpy(raw[k]).to(dtype) for k in ("feat_render", "feat_real", "h_feat", "cxt_feat")}
    h, w = t["feat_render"].shape[-2:]
    return dict(feat1=t["feat_render"], feat2=t["feat_real"], flow=torch.zeros(B, 2, h, w, dtype=dtype),
                h_feat=t["h_feat"], cxt_feat=t["cxt_feat"])


def convex_upsample(x, logits, logit_scale=0.25, value_scale=1.0, scale=8):
    """x [N, C, h, w], raw logits [N, 9·scale², h, w] → [N, C, scale·h, scale·w]: per sub-pixel
    (sy, sx) a softmax over the 3×3 neighbourhood (channel k·scale² + sy·scale + sx, k = ky·3 + kx)
    weighs the zero-padded neighbours of x, scaled by value_scale."""
    N, C, h, w = x.shape
    wgt = torch.softmax((logit_scale * logits).view(N, 1, 9, scale * scale, h, w), dim=2)
    nb = F.unfold(value_scale * x, 3, padding=1).view(N, C, 9, 1, h, w)
    up = (wgt * nb).sum(dim=2).view(N, C, scale, scale, h, w)
    return up.permute(0, 1, 4, 2, 5, 3).reshape(N, C, scale * h, scale * w)


def raft_forward(sd, feat1, feat2, flow, h_feat, cxt_feat, iters, occlusion=True, convex=True,
                 num_levels=4, radius=4):
    """→ dict(upflow=[...], upocc=[...] (empty without the occlusion head), lr_flow=[...])."""
    scale = 2 ** (num_levels - 1)
    pyr = orc.corr_pyramid(feat1, feat2, num_levels)
    out = dict(upflow=[], upocc=[], lr_flow=[])
    for _ in range(iters):
        corr = orc.corr_lookup(pyr, flow, radius)
        x = torch.cat([cxt_feat, orc.motion_encoder(sd, corr, flow)], 1)
        h_feat = orc.conv_gru(sd, h_feat, x)
        flow = flow + orc.xhead(sd, h_feat, "flow_pred", "flow")
        out["lr_flow"].append(flow)
        occ = torch.sigmoid(orc.xhead(sd, h_feat, "occlusion_pred", "mask")) if occlusion else None
        if convex:
            logits = orc.xhead(sd, h_feat, "mask_pred", "mask")
            out["upflow"].append(convex_upsample(flow, logits, value_scale=float(scale)))
            if occlusion:
                out["upocc"].append(convex_upsample(occ, logits))
        else:
            out["upflow"].append(scale * orc.upsample(flow, scale))
            if occlusion:
                out["upocc"].append(orc.upsample(occ, scale))
    return out


def mean_epe(ref, got):
    """Per-sample mean endpoint error (cal_epe 'mean'), the largest over the batch."""
    return float(orc.cal_epe_mean(ref, got).max())
