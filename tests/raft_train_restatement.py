"""Test-side helper (not a test): a pure-torch restatement of the RAFT baseline's TRAINING data flow
on the oracle's functions — ``RAFTRefinerFlowMask.loss`` (models/refiner/
raft_refiner_flow_mask.py:167-220) over ``RAFTDecoderMask.forward`` / ``RAFTDecoder.forward`` with
the per-iteration ``flow.detach()`` — the gather-form adjoint of the convex upsampling that
``scflow_convex_upsample_bwd`` implements, and what the RAFT training tests share (the fixture of
``tests/golden/make_golden_raft_train.py``, the three variants, the product refiners holding the
fixture's weights, the comparison against the fixture).

``tests/test_raft_train_host.py`` pins the restatement to the fixture, i.e. to the reference's own
modules.
"""
import os
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from oracle import scflow_oracle as orc
from tests import raft_restatement as rr
from tests.helpers import GOLDEN, encoder_state_dict

# tag → (refiner type, decoder type, state-dict tag of raft_restatement, decoder overrides)
VARIANTS = {"mask": ("RAFTRefinerFlowMask", "RAFTDecoderMask", "mask", {}),
            "plain": ("RAFTRefinerFlow", "RAFTDecoder", "plain", {}),
            "bilinear": ("RAFTRefinerFlowMask", "RAFTDecoderMask", "mask",
                         dict(convex_unsample_flow=False))}
BIAS_GRADS = ("mask_pred.predict_layer.bias", "flow_pred.predict_layer.bias",
              "occlusion_pred.predict_layer.bias")


@lru_cache(maxsize=None)
def raft_train_golden():
    with np.load(os.path.join(GOLDEN, "golden_raft_train_b2_s256_it3.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def fixture_meta():
    """(B, S, iters, seed, labels, dict(gamma, flow_weight, occ_weight, max_flow))."""
    g = raft_train_golden()
    B, S, iters, seed, *labels = (int(x) for x in g["meta"])
    gamma, fw, ow, mf = (float(x) for x in g["loss_cfg"])
    return B, S, iters, seed, labels, dict(gamma=gamma, flow_weight=fw, occ_weight=ow, max_flow=mf)


# ------------------------------------------------------------------ weights and product modules
def train_state_dict(tag, dtype=torch.float32):
    """Flat oracle state dict: the decoder's keys (seed 0 + the fixture's gain) unprefixed, the
    shared IN feature encoder (seed 1) under both names, the BN context encoder (seed 2)."""
    sd = dict(rr.raft_state_dict(VARIANTS[tag][2], seed=0, gain=float(raft_train_golden()["gain"]),
                                 dtype=dtype))
    for prefix, norm, seed in (("real_encoder.", "IN", 1), ("render_encoder.", "IN", 1),
                               ("context.", "BN", 2)):
        sd.update(encoder_state_dict(norm, seed, prefix, dtype))
    return sd


def model_cfg(tag, iters, **over):
    """The model block of the reference's configs/refine_models/raft.py with its loss configs."""
    kind, dec_kind, _, dec_over = VARIANTS[tag]
    _, _, _, _, _, lc = fixture_meta()
    enc = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic",
               norm_cfg=dict(type="IN"))
    ctx = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic",
               norm_cfg=dict(type="BN"))
    cfg = dict(type=kind, cxt_channels=128, h_channels=128, seperate_encoder=False,
               max_flow=lc["max_flow"], filter_invalid_flow_by_mask=True,
               filter_invalid_flow_by_depth=False, encoder=enc, cxt_encoder=ctx, freeze_bn=False,
               train_cfg=dict(), test_cfg=dict(iters=12),
               decoder=dict(type=dec_kind, **rr.raft_decoder_cfg(iters, **dec_over)))
    loss = dict(type="SequenceLoss", gamma=lc["gamma"],
                loss_func_cfg=dict(type="RAFTLoss", loss_weight=lc["flow_weight"],
                                   max_flow=lc["max_flow"]))
    if kind == "RAFTRefinerFlowMask":
        cfg.update(flow_loss_cfg=loss, occlusion_loss_cfg=dict(
            type="SequenceLoss", gamma=lc["gamma"],
            loss_func_cfg=dict(type="L1Loss", loss_weight=lc["occ_weight"])))
    else:
        cfg.update(loss_cfg=loss)
    cfg.update(over)
    return cfg


def build_train_refiner(tag, iters=None, dtype=torch.float32, **over):
    """The product refiner of a variant in train mode with the fixture's weights (CPU)."""
    from scflow_amd import MODELS
    iters = fixture_meta()[2] if iters is None else iters
    r = MODELS.build(model_cfg(tag, iters, **over))
    full = {(k if k.startswith(("real_encoder.", "render_encoder.", "context.")) else "decoder." + k): v
            for k, v in train_state_dict(tag).items()}
    missing, unexpected = r.load_state_dict(full, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), missing
    return r.to(dtype).train()


# ------------------------------------------------------------------ the restatement
def raft_train_forward(sd, batch, iters, occlusion=True, convex=True, gamma=0.8, flow_weight=1.0,
                       occ_weight=100.0, max_flow=400., num_levels=4, radius=4):
    """``batch``: the keys of ``synthetic.make_train_batch`` (tensors).  → dict(loss, loss_flow,
    loss_occ (None without the occlusion head), seq_flow, seq_occ, lr_flow, upflow, upocc,
    gt_flow), autograd graph attached to ``sd``'s tensors."""
    dt = batch["render_images"].dtype
    feat1, feat2, h_feat, cxt_feat = orc.extract_feat(sd, batch["render_images"], batch["real_images"],
                                                      train=True)
    scale = 2 ** (num_levels - 1)
    N, _, h, w = feat1.shape
    pyr = orc.corr_pyramid(feat1, feat2, num_levels)
    flow = torch.zeros(N, 2, h, w, dtype=dt)
    upflow, upocc, lr_flow = [], [], []
    for _ in range(iters):
        flow = flow.detach()  # raft_decoder.py:441 / raft_decoder_mask.py:183
        corr = orc.corr_lookup(pyr, flow, radius)
        x = torch.cat([cxt_feat, orc.motion_encoder(sd, corr, flow)], 1)
        h_feat = orc.conv_gru(sd, h_feat, x)
        flow = flow + orc.xhead(sd, h_feat, "flow_pred", "flow")
        lr_flow.append(flow)
        occ = torch.sigmoid(orc.xhead(sd, h_feat, "occlusion_pred", "mask")) if occlusion else None
        if convex:
            logits = orc.xhead(sd, h_feat, "mask_pred", "mask")
            upflow.append(rr.convex_upsample(flow, logits, value_scale=float(scale)))
            if occlusion:
                upocc.append(rr.convex_upsample(occ, logits))
        else:
            upflow.append(scale * orc.upsample(flow, scale))
            if occlusion:
                upocc.append(orc.upsample(occ, scale))
    with torch.no_grad():
        depth, K = batch["depth"].to(dt), batch["internel_k"].to(dt)
        pts, valid = orc.lift_points(depth, K, batch["ref_rotation"].to(dt),
                                     batch["ref_translation"].to(dt))
        gt_flow = orc.pose_flow(batch["gt_rotation"].to(dt), batch["gt_translation"].to(dt), K, pts,
                                valid, max_flow)
        gt_flow = orc.filter_flow_by_mask(gt_flow, batch["gt_masks"], max_flow)
        render_mask = (depth > 0).to(dt)
        gt_occ = (torch.sum(gt_flow, dim=1) < max_flow).to(dt)
    seq_flow = [orc.raft_loss(f, gt_flow, render_mask, flow_weight, max_flow) for f in upflow]
    loss_flow = orc.sequence_loss(seq_flow, gamma)
    seq_occ, loss_occ, loss = [], None, loss_flow
    if occlusion:
        seq_occ = [orc.l1_loss(o[:, 0], gt_occ, occ_weight) for o in upocc]
        loss_occ = orc.sequence_loss(seq_occ, gamma)
        loss = loss_flow + loss_occ
    return dict(loss=loss, loss_flow=loss_flow, loss_occ=loss_occ, seq_flow=seq_flow, seq_occ=seq_occ,
                lr_flow=lr_flow, upflow=upflow, upocc=upocc, gt_flow=gt_flow)


def convex_upsample_adjoint(x, logits, occ, g_flow, g_occ, logit_scale=0.25, value_scale=8.0):
    """The gather form of the convex upsampling's adjoint, NCHW: x [N, 2, h, w], raw logits
    [N, 576, h, w], occ [N, 1, h, w] or None, g_flow [N, 2, 8h, 8w], g_occ [N, 1, 8h, 8w] or None →
    (dx, dlogits, docc or None).  With k = ky·3 + kx, s = sy·8 + sx and w_k = softmax_k:
      dw_k[p][s]   = Σ_c vs_c · v_c[nb(p,k)] · g_c[p][s]           (out-of-map neighbours: 0)
      dlogits      = logit_scale · w_k · (dw_k − Σ_j w_j · dw_j)
      dv_c[q]      = vs_c · Σ_k T_c[q − (ky−1, kx−1)][k],  T_c[p][k] = Σ_s w_k[p][s] · g_c[p][s]."""
    N, _, h, w = x.shape
    wk = torch.softmax((logit_scale * logits).view(N, 9, 64, h, w), dim=1)

    def sub(g):  # [N, C, 8h, 8w] → [N, C, 64, h, w]
        C = g.shape[1]
        return g.view(N, C, h, 8, w, 8).permute(0, 1, 3, 5, 2, 4).reshape(N, C, 64, h, w)

    terms = [(x, sub(g_flow), value_scale)]
    if occ is not None:
        terms.append((occ, sub(g_occ) if g_occ is not None else torch.zeros_like(sub(g_flow)[:, :1]),
                      1.0))
    dw = 0
    for v, g, vs in terms:
        C = v.shape[1]
        nbv = F.unfold(v, 3, padding=1).view(N, C, 9, 1, h, w)
        dw = dw + (vs * nbv * g[:, :, None]).sum(1)  # [N, 9, 64, h, w]
    dlogits = logit_scale * wk * (dw - (wk * dw).sum(1, keepdim=True))
    outs = []
    for v, g, vs in terms:
        T = (wk[:, None] * g[:, :, None]).sum(3)  # [N, C, 9, h, w]
        dv = torch.zeros_like(v)
        for k in range(9):
            dy, dx_ = k // 3 - 1, k % 3 - 1
            Tp = F.pad(T[:, :, k], (1, 1, 1, 1))
            dv = dv + Tp[:, :, 1 - dy:1 - dy + h, 1 - dx_:1 - dx_ + w]
        outs.append(vs * dv)
    return outs[0], dlogits.reshape(N, 576, h, w), (outs[1] if occ is not None else None)


# ------------------------------------------------------------------ comparison with the fixture
def fixture_name(n):
    """A product parameter name → the fixture's (the shared encoder is ``encoder.`` there)."""
    return "encoder." + n.split(".", 1)[1] if n.startswith(("real_encoder.", "render_encoder.")) else n


def check_against_fixture(tag, res, refiner):
    """``raft_refiner_train_forward``'s result (after ``backward``) against the fixture, with the
    tolerances of tests/test_gpu_train.py test_train_forward_backward_matches_reference_fixture:
    losses rtol 1e-4; low-resolution flows mean EPE ≤ 1e-3 px; every gradient norm within 1e-3 of
    the decoder's largest norm (decoder) / 2e-2 of the encoders' largest (encoders) + 1e-3
    relative, every fixture name exactly once; the stored bias gradients elementwise within 1e-3
    of their largest magnitude."""
    g = raft_train_golden()
    want = g[f"{tag}_losses"]
    got = [res["loss"].item(), res["loss_flow"].item()] + \
        ([] if res["loss_occ"] is None else [res["loss_occ"].item()])
    print(f"{tag}: losses {got} vs fixture {want.tolist()}")
    assert len(got) == len(want)
    np.testing.assert_allclose(got, want, rtol=1e-4)
    np.testing.assert_allclose([v.item() for v in res["seq_flow_losses"]], g[f"{tag}_seq_flow"], rtol=1e-4)
    np.testing.assert_allclose([v.item() for v in res["seq_occ_losses"]], g[f"{tag}_seq_occ"], rtol=1e-4)
    lr = g[f"{tag}_lr_flow"]
    assert len(res["outs"][2]) == len(lr)
    for i, f in enumerate(res["outs"][2]):  # channels-last [N, h, w, 2]
        epe = rr.mean_epe(torch.from_numpy(lr[i]), f.detach().float().cpu().permute(0, 3, 1, 2))
        print(f"{tag}: iteration {i}: low-resolution flow mean EPE {epe:.3e} px")
        assert epe <= rr.EPE_TOL, i
    ref = dict(zip([str(n) for n in g[f"{tag}_grad_names"]], g[f"{tag}_grad_norms"]))
    dec_max = np.nanmax([v for k, v in ref.items() if k.startswith("decoder.")])
    enc_max = np.nanmax([v for k, v in ref.items() if not k.startswith("decoder.")])
    seen, worst = set(), 0.0
    for n, p in dict(refiner.named_parameters(remove_duplicate=False)).items():
        key = fixture_name(n)
        if key in seen:  # the shared encoder under its second name
            continue
        seen.add(key)
        rv = ref[key]
        if np.isnan(rv):  # no gradient in the reference either (mask_pred, bilinear variant)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert p.grad is not None, f"{n}: no gradient"
        gv = float(p.grad.double().norm())
        tol = (1e-3 * dec_max if key.startswith("decoder.") else 2e-2 * enc_max) + 1e-3 * rv
        worst = max(worst, abs(gv - rv) / tol)
        assert abs(gv - rv) <= tol, f"{n}: {gv:.6e} vs reference {rv:.6e}"
    assert seen == set(ref), set(ref) ^ seen
    print(f"{tag}: {len(seen)} gradient norms, worst at {worst:.3f} of its tolerance")
    for b in BIAS_GRADS:
        k = f"{tag}_grad_{b}"
        if k not in g:
            continue
        got_b = dict(refiner.named_parameters())["decoder." + b].grad.detach().double().cpu().numpy()
        err = float(np.abs(got_b - g[k]).max())
        bound = 1e-3 * float(np.abs(g[k]).max())
        print(f"{tag}: {b} gradient max error {err:.3e} (bound {bound:.3e})")
        assert err <= bound, b
