"""GPU: RAFTRefinerFlow / RAFTRefinerFlowMask.get_flow (images → encoders → RAFT decoder, the
device-side path) against the oracle's feature extraction + the RAFT restatement, B=2, 256²,
4 iterations, the decoder tests' gates (upflow mean EPE ≤ 1e-3 px, occlusion atol 1e-4)."""
import numpy as np
import pytest
import torch

from tests import raft_restatement as rr
from tests.helpers import encoder_state_dict, refine_inputs

orc = pytest.importorskip("oracle.scflow_oracle")

ITERS = 4


def model_cfg(kind, seperate):
    """The model block of the reference's configs/refine_models/raft.py:4-75 (loss configs kept as
    given; no checkpoint)."""
    enc = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic",
               norm_cfg=dict(type="IN"))
    ctx = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic",
               norm_cfg=dict(type="BN"))
    cfg = dict(type=kind, cxt_channels=128, h_channels=128, seperate_encoder=seperate, max_flow=400.,
               filter_invalid_flow_by_mask=True, filter_invalid_flow_by_depth=False, encoder=enc,
               cxt_encoder=ctx, freeze_bn=False, train_cfg=dict(), test_cfg=dict(iters=12))
    loss = dict(type="SequenceLoss", gamma=0.8,
                loss_func_cfg=dict(type="RAFTLoss", loss_weight=1.0, max_flow=400.))
    if kind == "RAFTRefinerFlowMask":
        cfg.update(decoder=dict(type="RAFTDecoderMask", **rr.raft_decoder_cfg(ITERS)),
                   flow_loss_cfg=loss,
                   occlusion_loss_cfg=dict(type="SequenceLoss", gamma=0.8,
                                           loss_func_cfg=dict(type="L1Loss", loss_weight=100.)))
    else:
        cfg.update(decoder=dict(type="RAFTDecoder", **rr.raft_decoder_cfg(ITERS)), loss_cfg=loss)
    return cfg


def build_refiner(kind, seperate):
    """→ (module on the GPU, the flat oracle state dict it holds).  Feature encoder seed 1 (the
    rendered images' own encoder seed 3 when separate), context seed 2, decoder seed 0 + gain."""
    from scflow_amd import MODELS
    r = MODELS.build(model_cfg(kind, seperate))
    assert r.test_iter_num == 12 and (r.real_encoder is r.render_encoder) == (not seperate)
    tag = "mask" if kind == "RAFTRefinerFlowMask" else "plain"
    sd = dict(rr.raft_state_dict(tag, seed=0))
    full = {"decoder." + k: v for k, v in sd.items()}
    for prefix, norm, seed in (("real_encoder.", "IN", 1),
                               ("render_encoder.", "IN", 3 if seperate else 1),
                               ("context.", "BN", 2)):
        part = encoder_state_dict(norm, seed, prefix)
        sd.update(part)
        full.update(part)
    missing, unexpected = r.load_state_dict(full, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), missing
    return r.eval().cuda(), sd


@pytest.mark.gpu
@pytest.mark.parametrize("kind,seperate", [("RAFTRefinerFlowMask", False),
                                           ("RAFTRefinerFlowMask", True),
                                           ("RAFTRefinerFlow", False)])
def test_get_flow_matches_oracle(kind, seperate):
    inp = refine_inputs(2, 256, seed=13)
    r, sd = build_refiner(kind, seperate)
    out = r.get_flow(inp["render_images"].cuda(), inp["real_images"].cuda())
    torch.cuda.synchronize()
    masked = kind == "RAFTRefinerFlowMask"
    upflow, upocc = (out if masked else (out, None))
    assert len(upflow) == ITERS
    feat_render, feat_real, h_feat, cxt_feat = orc.extract_feat(sd, inp["render_images"],
                                                                inp["real_images"])
    flow0 = torch.zeros(2, 2, *feat_real.shape[-2:])
    ref = rr.raft_forward(sd, feat_render, feat_real, flow0, h_feat, cxt_feat, iters=ITERS,
                          occlusion=masked)
    for i in range(ITERS):
        epe = rr.mean_epe(ref["upflow"][i], upflow[i].cpu())
        print(f"{kind} seperate={seperate} iteration {i}: upflow mean EPE {epe:.3e} px")
        assert epe <= rr.EPE_TOL, i
        if masked:
            np.testing.assert_allclose(upocc[i].cpu().numpy(), ref["upocc"][i].numpy(), atol=1e-4)


@pytest.mark.gpu
def test_get_flow_warm_start_equals_decoder_on_extracted_features():
    """``init_flow`` is at the feature resolution; the fused path (shared encoder over
    cat[real, render], context written into the GRU buffer) is the same arithmetic as extract_feat
    + the decoder's NCHW forward: equal up to a launch's tiling of 2B against B images (EPE ≤ 1e-5
    px, a hundredth of the gate; occlusion 1e-6)."""
    inp = refine_inputs(2, 256, seed=13)
    r, _ = build_refiner("RAFTRefinerFlowMask", False)
    g = torch.Generator().manual_seed(8)
    init = ((torch.rand(2, 2, 32, 32, generator=g) - 0.5) * 3).cuda()
    render, real = inp["render_images"].cuda(), inp["real_images"].cuda()
    up_a, occ_a = r.get_flow(render, real, init_flow=init)
    up_b, occ_b = r.decoder(*r.extract_feat(render, real)[:2], init, *r.extract_feat(render, real)[2:])
    torch.cuda.synchronize()
    for a, b in zip(up_a, up_b):
        assert rr.mean_epe(b.cpu(), a.cpu()) <= 1e-5
    for a, b in zip(occ_a, occ_b):
        torch.testing.assert_close(a, b, rtol=0, atol=1e-6)


def test_refiner_rejects_cpu_tensors():
    from scflow_amd import MODELS
    from scflow_amd._lib import ScflowError
    r = MODELS.build(model_cfg("RAFTRefinerFlowMask", False))
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ScflowError):
        r.get_flow(x, x)
