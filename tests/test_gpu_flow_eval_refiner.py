"""GPU: ``val_step`` of SCFlowRefiner, RAFTRefinerFlowMask and RAFTRefinerFlow at B = 2, 256², two
iterations (``test_cfg['iters']``), synthetic weights — 256² because the decoders' kernels are
built and validated for feature maps 32 or 64 wide, so 64² and 128² patches are
not shapes these refiners run at; the flow-validation kernels themselves are tested at 8², 20 × 36
and 64² in ``test_gpu_flow_eval_ops.py``.  Checked: the reference's keys, ``num_samples``, and
values equal to the float64 restatement's ``eval_epe_and_occ`` of that refiner's own ``get_pose`` /
``get_flow`` outputs against the GT flow of ``flow_eval.gt_flow`` (whose bits and decisions
``test_gpu_flow_eval_ops.py`` pins).  With and without ``gt_masks``; ``decoder.iters`` and every
module's training mode are left as they were.

Gates: an error mean may deviate, relatively, by four times the relative deviation of the
reference's own float32 ``cal_epe`` from its float64 run at 64² (``golden_flow_eval.npz``
``dev_fixture`` over its mean EPE: the rounding of a float32 sum scales with the sum); an accuracy
by the share of pixels within 1e-3 px of its threshold; ``occ`` by 2^-25 (see the ops test)."""
import os

import numpy as np
import pytest
import torch

from tests import flow_eval_restatement as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_flow_eval.npz")
B, S, ITERS, TRAIN_ITERS = 2, 256, 2, 5
KEYS = ["mean", "1px", "3px", "5px"]
OCC_TOL = 2.0 ** -25


def build(kind):
    from scflow_amd import MODELS, synthetic
    from tests import raft_restatement as rr
    from tests.test_gpu_decoder import decoder_cfg
    enc = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic",
               norm_cfg=dict(type="IN"))
    ctx = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic",
               norm_cfg=dict(type="BN"))
    cfg = dict(type=kind, cxt_channels=128, h_channels=128, seperate_encoder=False, max_flow=400.,
               encoder=enc, cxt_encoder=ctx, test_cfg=dict(iters=ITERS))
    if kind == "SCFlowRefiner":
        cfg.update(decoder=dict(type="SCFlowDecoder", **decoder_cfg(TRAIN_ITERS)))
    else:
        dec = "RAFTDecoderMask" if kind == "RAFTRefinerFlowMask" else "RAFTDecoder"
        cfg.update(decoder=dict(type=dec, **rr.raft_decoder_cfg(TRAIN_ITERS)))
    r = MODELS.build(cfg)
    synthetic.fill_module_(r, seed=4)
    return r.cuda()


def batch(with_masks=True):
    from scflow_amd import synthetic
    out = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
           for k, v in synthetic.make_train_batch(B, S, seed=3).items()}
    if not with_masks:
        del out["gt_masks"]
    return out


def predictions(r, kind, b):
    """The refiner's own last flows (and occlusion) at ITERS iterations, in eval mode (the HIP
    encoders take no BatchNorm in training mode): {prefix: flow}, occ."""
    r.decoder.iters = ITERS
    modes = [(m, m.training) for m in r.modules()]
    r.eval()
    try:
        if kind == "SCFlowRefiner":
            out = r.get_pose(b["render_images"], b["real_images"], b["ref_rotation"], b["ref_translation"],
                             b["depth"], b["internel_k"], b["label"])
            return {"epe": out[1][-1], "pose_epe": out[0][-1]}, None
        out = r.get_flow(b["render_images"], b["real_images"])
        flows, occs = out if isinstance(out, tuple) else (out, None)
        return {"epe": flows[-1]}, None if occs is None else occs[-1]
    finally:
        r.decoder.iters = TRAIN_ITERS
        for m, t in modes:
            m.training = t


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("kind", ["SCFlowRefiner", "RAFTRefinerFlowMask", "RAFTRefinerFlow"])
def test_val_step(kind, mode):
    from scflow_amd import flow_eval
    gold = np.load(GOLD)
    rel = 4 * float(gold["dev_fixture"][0]) / float(gold["epe_total_mean_nomask"][0])
    r = build(kind)
    r = r.train() if mode == "train" else r.eval()
    flags = [m.training for m in r.modules()]
    for with_masks in (True, False):
        b = batch(with_masks)
        res = r.val_step(b)
        assert r.decoder.iters == TRAIN_ITERS and [m.training for m in r.modules()] == flags
        assert set(res) == {"log_vars", "num_samples"} and res["num_samples"] == B
        log = res["log_vars"]
        assert all(isinstance(v, float) and np.isfinite(v) for v in log.values())
        preds, occ = predictions(r, kind, b)
        flow, noc = flow_eval.gt_flow(b["depth"], b["internel_k"], b["ref_rotation"], b["ref_translation"],
                                      b["gt_rotation"], b["gt_translation"], 400.,
                                      gt_mask=b.get("gt_masks"))
        flow, noc = flow.cpu(), (noc.cpu() if with_masks else None)
        want, near = {}, {}
        for prefix, pred in preds.items():
            w = fr.eval_epe_and_occ(pred.cpu(), None if occ is None else occ.cpu(), flow, noc, 400.,
                                    "total_mean", noc_without_mask=kind == "RAFTRefinerFlow",
                                    prefix=prefix)
            for k, v in w.items():
                want.setdefault(k, float(v))
                st = fr.epe_stats(noc if ("noc" in k and noc is not None) else flow, pred.cpu(), None, 400.)
                near[k] = float(st["near"].sum()) / float(st["count"].sum() + 1e-10)
        # the reference's keys, in its order
        expect = [f"epe_{k}" for k in KEYS]
        if with_masks or kind == "RAFTRefinerFlow":
            expect += [f"epe_noc_{k}" for k in KEYS]
        if kind == "RAFTRefinerFlowMask":
            expect += ["occ"]
        if kind == "SCFlowRefiner":
            expect += [f"pose_epe_{k}" for k in KEYS] + ([f"pose_epe_noc_{k}" for k in KEYS] if with_masks else [])
        assert list(log) == expect, list(log)
        for k in expect:
            tol = OCC_TOL if k == "occ" else rel * abs(want[k]) if k.endswith("mean") else near[k] + 1e-12
            print(f"{kind} {mode} masks={with_masks} {k}: val_step {log[k]:.9g}, restatement {want[k]:.9g}, "
                  f"gate {tol:.3e}")
            assert abs(log[k] - want[k]) <= tol, k
        if kind == "RAFTRefinerFlow" and not with_masks:
            assert all(log[f"epe_noc_{k}"] == log[f"epe_{k}"] for k in KEYS)
        if kind == "SCFlowRefiner" and not with_masks:
            assert not any("noc" in k for k in log)
