"""Training fixture of the RAFT baseline from the REFERENCE's own modules in train mode, with
``make_golden``'s shims and stand-ins and ``make_golden_raft``'s decoder configuration and gain.

    python tests/golden/make_golden_raft_train.py

writes ``golden_raft_train_b2_s256_it3.npz``.  The data flow is ``RAFTRefinerFlowMask.loss``
(models/refiner/raft_refiner_flow_mask.py:167-220) restated on the reference's modules as
``make_golden.gen_train`` restates ``SCFlowRefiner.loss``: shared IN feature encoder (seed 1), BN
context encoder (seed 2, batch statistics), the RAFT decoder (seed 0,
``mask_pred.predict_layer.weight × GAIN``), the GT flow from
``pose.get_flow_from_delta_pose_and_depth`` + ``flow.filter_flow_by_mask``, the occlusion target
``gt_flow.sum(1) < max_flow`` and the losses of configs/refine_models/raft.py:
``SequenceLoss(RAFTLoss, weight 1)`` on the ×8 flows plus ``SequenceLoss(L1Loss, weight 100)`` on
the ×8 occlusions.  The batch is ``make_train_batch(2, 256, seed=5, labels=[0, 1])``, 3 iterations.

Three variants (keys prefixed ``mask_`` / ``plain_`` / ``bilinear_``):
* ``mask``: RAFTDecoderMask, convex upsampling;
* ``plain``: RAFTDecoder, convex upsampling — ``RAFTRefinerFlow.loss`` cannot run as the reference
  writes it (raft_refiner_flow.py:184 unpacks the list of flows into three names); its evident
  intent, the flow sequence loss alone, is what is recorded;
* ``bilinear``: RAFTDecoderMask with ``convex_unsample_flow=False``.

Per variant: the losses, both per-iteration loss lists, the GT-flow statistics (as ``gen_train``
stores them), the low-resolution flow after every iteration, every parameter's name and gradient
norm (NaN: no gradient) and the whole gradients of the three predictors' biases — a permuted
``dlogits`` keeps the weight's gradient norm, the elementwise bias gradient catches it.

Every variant runs in float32 and in float64 (the reference's ``.float()`` cast in the lookup kept
at the run's precision, as ``make_golden_raft`` does).  The generator refuses to write unless every
iteration's softmax passes ``make_golden_raft.flat_fraction ≥ 0.5`` and the float64 run agrees
with the float32 run to 1e-6 relative on the losses and to a tenth of the GPU test's tolerances on
every gradient norm.  The float64 run's values are the ones stored (the low-resolution flows
rounded to float32): they are the more exact statement of what the reference computes, and a
float64 restatement can be pinned to them far inside the GPU tolerances.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_raft as mgr  # noqa: E402
from scflow_amd import synthetic  # noqa: E402

NAME = "golden_raft_train_b2_s256_it3"
B, S, ITERS, SEED, LABELS = 2, 256, 3, 5, (0, 1)
MAX_FLOW, GAMMA, FLOW_WEIGHT, OCC_WEIGHT = 400., 0.8, 1.0, 100.
BIAS_GRADS = ("mask_pred.predict_layer.bias", "flow_pred.predict_layer.bias",
              "occlusion_pred.predict_layer.bias")
# the GPU test's gradient-norm tolerances (tests/test_gpu_train.py): share of the part's largest norm
DEC_TOL, ENC_TOL, REL_TOL = 1e-3, 2e-2, 1e-3
VARIANTS = (("mask", "mask", {}), ("plain", "plain", {}),
            ("bilinear", "mask", dict(convex_unsample_flow=False)))


def run_variant(ref, L, kind, over, dtype):
    """→ dict of the variant's results (tensors detached, in ``dtype``)."""
    raw = synthetic.make_train_batch(B, S, seed=SEED, labels=list(LABELS))
    t = {k: mg.t32(v) for k, v in raw.items()}
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in t.items()}
    enc = mg.build_encoder(ref, "IN", 1).to(dtype).train()
    ctx = mg.build_encoder(ref, "BN", 2).to(dtype).train()
    cls = ref.raft_mask.RAFTDecoderMask if kind == "mask" else ref.raft.RAFTDecoder
    dec = cls(**dict(mgr.raft_decoder_cfg(ITERS), **over))
    synthetic.fill_module_(dec, seed=mgr.W_SEED)
    with torch.no_grad():
        dec.mask_pred.predict_layer.weight.mul_(mgr.GAIN)
    dec = dec.to(dtype).train()

    lr_flows, logits = [], []
    name = "upsample_flow" if hasattr(dec, "upsample_flow") else "_upsample"
    orig = getattr(dec, name)

    def watch(flow, mask=None):
        lr_flows.append(flow.detach().clone())
        if mask is not None:
            logits.append(mask.detach().clone())
        return orig(flow, mask)
    setattr(dec, name, watch)

    # the reference casts the lookup with `.float()` (corr_lookup.py:136): the float64 run keeps
    # its precision instead (as make_golden_raft.run does)
    to_float = torch.Tensor.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        real_feat = enc(t["real_images"])
        render_feat = enc(t["render_images"])
        cxt = ctx(t["render_images"])
        h_feat, cxt_feat = torch.split(cxt, [128, 128], dim=1)
        h_feat, cxt_feat = torch.tanh(h_feat), torch.relu(cxt_feat)
        init_flow = torch.zeros(B, 2, *real_feat.shape[-2:], dtype=dtype)
        out = dec(render_feat, real_feat, init_flow, h_feat, cxt_feat)
    finally:
        torch.Tensor.float = to_float
    seq_flow, seq_occ = out if kind == "mask" else (out, None)
    depth = t["depth"]
    gt_flow = ref.pose.get_flow_from_delta_pose_and_depth(
        t["ref_rotation"], t["ref_translation"], t["gt_rotation"], t["gt_translation"], depth,
        t["internel_k"], invalid_num=MAX_FLOW)
    gt_flow = L.flow.filter_flow_by_mask(gt_flow, t["gt_masks"], invalid_num=MAX_FLOW)
    rendered_masks = (depth > 0).to(dtype)  # base_refiner.py:191
    gt_occ = (torch.sum(gt_flow, dim=1, keepdim=False) < MAX_FLOW).to(dtype)
    flow_loss = L.seq.SequenceLoss(gamma=GAMMA, loss_func_cfg=dict(
        type=L.seq.RAFTLoss, loss_weight=FLOW_WEIGHT, max_flow=MAX_FLOW))
    lf, lf_seq = flow_loss(seq_flow, gt_flow=gt_flow, valid=rendered_masks)
    loss, lo, lo_seq = lf, None, []
    if seq_occ is not None:
        occ_loss = L.seq.SequenceLoss(gamma=GAMMA, loss_func_cfg=dict(type=L.seq.L1Loss,
                                                                      loss_weight=OCC_WEIGHT))
        lo, lo_seq = occ_loss([o.squeeze(dim=1) for o in seq_occ], gt_mask=gt_occ,
                              valid=rendered_masks)
        loss = lf + lo
    loss.backward()
    names, norms, grads = [], [], {}
    for prefix, mod in (("encoder.", enc), ("context.", ctx), ("decoder.", dec)):
        for n, p in mod.named_parameters():
            names.append(prefix + n)
            norms.append(np.nan if p.grad is None else p.grad.double().norm().item())
            if prefix == "decoder." and n in BIAS_GRADS and p.grad is not None:
                grads[n] = p.grad.detach().clone()
    mag = gt_flow.pow(2).sum(1).sqrt()
    valid_share = float(((rendered_masks >= 0.5) & (mag < MAX_FLOW)).double().mean())
    return dict(losses=[loss.item(), lf.item()] + ([] if lo is None else [lo.item()]),
                seq_flow=[x.item() for x in lf_seq], seq_occ=[x.item() for x in lo_seq],
                gt_flow_stats=[gt_flow.double().sum().item(), (gt_flow >= MAX_FLOW).sum().item(),
                               gt_flow[gt_flow < MAX_FLOW].double().abs().sum().item()],
                lr_flow=torch.stack(lr_flows), logits=logits, names=names, norms=np.array(norms),
                grads=grads, valid_share=valid_share)


def check_conditioning(tag, r32, r64):
    """Refusal 2: float32 against float64."""
    np.testing.assert_allclose(r32["losses"], r64["losses"], rtol=1e-6, err_msg=f"{tag}: losses")
    assert r32["names"] == r64["names"]
    n32, n64 = r32["norms"], r64["norms"]
    assert np.array_equal(np.isnan(n32), np.isnan(n64)), f"{tag}: gradient presence differs"
    dec = np.array([n.startswith("decoder.") for n in r64["names"]])
    dec_max, enc_max = np.nanmax(n64[dec]), np.nanmax(n64[~dec])
    tol = 0.1 * (np.where(dec, DEC_TOL * dec_max, ENC_TOL * enc_max) + REL_TOL * n64)
    ok = np.isnan(n64) | (np.abs(n32 - n64) <= tol)
    worst = np.nanmax(np.abs(n32 - n64) / tol)
    print(f"{tag}: float32 vs float64: loss rel diff "
          f"{abs(r32['losses'][0] - r64['losses'][0]) / abs(r64['losses'][0]):.2e}, worst gradient "
          f"norm difference {worst:.2e} of a tenth of the test tolerance")
    assert ok.all(), f"{tag}: ill-conditioned gradients: {[r64['names'][i] for i in np.where(~ok)[0]]}"


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref = mgr.load_raft(mg.load_reference())
    L = mg.load_losses(ref, synthetic.make_model_points(256))
    out = {"meta": np.array([B, S, ITERS, SEED, *LABELS]), "gain": np.array(mgr.GAIN),
           "loss_cfg": np.array([GAMMA, FLOW_WEIGHT, OCC_WEIGHT, MAX_FLOW])}
    for tag, kind, over in VARIANTS:
        r32 = run_variant(ref, L, kind, over, torch.float32)
        # refusal 1: a flat softmax would not tell a wrong channel order from the right one
        fracs = [mgr.flat_fraction(m) for m in r32["logits"]]
        if over.get("convex_unsample_flow", True):
            assert len(fracs) == ITERS
            print(f"{tag}: softmax flat fractions {[f'{f:.3f}' for f in fracs]}")
            assert min(fracs) >= mgr.FLAT_MIN_FRACTION, f"{tag}: flat or saturated softmax: {fracs}"
        r64 = run_variant(ref, L, kind, over, torch.float64)
        check_conditioning(tag, r32, r64)
        missing = [n for n, v in zip(r64["names"], r64["norms"]) if np.isnan(v)]
        print(f"{tag}: float32 losses {r32['losses']}, float64 {r64['losses']}, "
              f"{len(r64['names'])} parameters, without gradient: {missing}, valid-pixel share "
              f"{r64['valid_share']:.3f}")
        # the float64 run is what is stored (the float32 run only admits it)
        out[f"{tag}_losses"] = np.array(r64["losses"])
        out[f"{tag}_seq_flow"] = np.array(r64["seq_flow"])
        out[f"{tag}_seq_occ"] = np.array(r64["seq_occ"])
        out[f"{tag}_gt_flow_stats"] = np.array(r64["gt_flow_stats"])
        out[f"{tag}_lr_flow"] = r64["lr_flow"].float().numpy()
        out[f"{tag}_flat_fraction"] = np.array(fracs)
        out[f"{tag}_grad_names"] = np.array(r64["names"])
        out[f"{tag}_grad_norms"] = r64["norms"]
        for n, g in r64["grads"].items():
            out[f"{tag}_grad_{n}"] = g.numpy()
    mgr.save(NAME, out)


if __name__ == "__main__":
    main()
