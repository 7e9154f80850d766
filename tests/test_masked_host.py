"""CPU: the occlusion-masked decoder (mask_flow / mask_corr, scflow_decoder.py:189-207) pinned on
the host — the oracle with both flags against the fixtures the reference itself produced
(tests/golden/make_golden_masked.py), the separation of masked from unmasked results, the C ABI's
new exports and the training path's flag check.

The masked e2e fixture is two files (``flow_pred_last`` is 1 MiB of incompressible floats and has
a file of its own: no fixture may exceed 1 MiB); ``masked_e2e_fixture`` joins them.
"""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, decoder_inputs, golden, oracle_state_dict, refiner_state_dict, t
from tests.test_train_host import train_batch

orc = pytest.importorskip("oracle.scflow_oracle")

E2E = "golden_e2e_masked_b2_s256_it4"
TRAIN = "golden_train_masked_b2_s256_it3"


@lru_cache(maxsize=None)
def masked_e2e_fixture():
    g = {}
    for name in (E2E + ".npz", E2E + "_flow_pred.npz"):
        with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files})
    return g


@lru_cache(maxsize=None)
def masked_train_fixture():
    with np.load(os.path.join(GOLDEN, TRAIN + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_masked_fixtures_have_the_unmasked_fixtures_keys():
    assert set(masked_e2e_fixture()) == set(golden("e2e"))
    with np.load(os.path.join(GOLDEN, "golden_train_b2_s256_it2.npz")) as z:
        assert set(masked_train_fixture()) == set(z.files)
    assert [int(v) for v in masked_e2e_fixture()["meta"]] == [2, 256, 4, 11]
    assert [int(v) for v in masked_train_fixture()["meta"][:3]] == [2, 256, 3]
    for name in (E2E + ".npz", E2E + "_flow_pred.npz", TRAIN + ".npz"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= 1 << 20, name
    # same inputs as the unmasked fixture, another result: the fixture exercises the masking
    a, b = masked_e2e_fixture(), golden("e2e")
    np.testing.assert_array_equal(a["sum_feat_render"], b["sum_feat_render"])
    assert np.abs(a["t"][-1] - b["t"][-1]).max() > 1e-2


def test_oracle_masked_decoder_matches_reference():
    """tests/test_oracle_golden.py::test_decoder_e2e_matches_reference's asserts, both flags."""
    g = masked_e2e_fixture()
    B, S, iters, seed = (int(v) for v in g["meta"])
    inp = decoder_inputs(B, S, seed, g)
    outs = orc.decoder_forward(oracle_state_dict(), **inp, iters=iters, mask_flow=True, mask_corr=True)
    fp, fpred, Rs, ts, masks, drs, dts = outs
    epe_pose = orc.cal_epe_mean(t(g["flow_pose_last"]), fp[-1])
    epe_pred = orc.cal_epe_mean(t(g["flow_pred_last"]), fpred[-1])
    assert float(epe_pose.max()) <= 1e-3, epe_pose
    assert float(epe_pred.max()) <= 1e-3, epe_pred
    np.testing.assert_allclose(torch.stack(Rs).numpy(), g["R"], atol=1e-5)
    np.testing.assert_allclose(torch.stack(ts).numpy(), g["t"], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(torch.stack(drs).numpy(), g["drot"], atol=1e-5)
    np.testing.assert_allclose(torch.stack(dts).numpy(), g["dt"], atol=1e-5)
    np.testing.assert_allclose(masks[-1].numpy(), g["mask_last"], atol=1e-5)
    assert g["flow_pose_absmean"][-1] > 0.05


def masked_train_decoder_forward(sd, feat_render, feat_real, h_feat, cxt_feat, ref_rotation,
                                 ref_translation, depth, internel_k, label, init_flow,
                                 invalid_flow_num=0.0, iters=8, train=True, **kw):
    """``orc.decoder_forward`` with mask_flow = mask_corr = True and detach_mask = True, composed
    from the oracle's own pieces.  The oracle's loop takes the two flags but its ``train`` mode
    restates only detach_flow / detach_pose / detach_depth_for_xy (its training entry never sets
    the flags), so the detach of the previous iteration's mask (scflow_decoder.py:195-196) is
    added here; everything else is the oracle's loop line for line."""
    assert train and not kw
    import torch.nn.functional as F
    dt = feat_render.dtype
    sd = {k: v.to(dt) if v.is_floating_point() else v for k, v in sd.items()}
    pyr = orc.corr_pyramid(feat_render, feat_real, 4)
    scale = 8
    N, H, W = depth.shape
    points, valid = orc.lift_points(depth.to(dt), internel_k.to(dt), ref_rotation.to(dt),
                                    ref_translation.to(dt))
    R, tr = ref_rotation.to(dt), ref_translation.to(dt)
    K = internel_k.to(dt)
    mask = F.interpolate(torch.ones(N, 1, H, W, dtype=dt), scale_factor=(1 / scale, 1 / scale),
                         mode="bilinear", align_corners=True)
    flow = init_flow.to(dt)
    h = h_feat
    outs = ([], [], [], [], [], [], [])
    for _ in range(iters):
        flow = flow.detach()
        mask = mask.detach()
        flow = orc.downsample_flow(flow, scale)
        corr = orc.corr_lookup(pyr, flow, 4) * mask
        motion = orc.motion_encoder(sd, corr, flow * mask, "ReLU")
        h = orc.conv_gru(sd, h, torch.cat([cxt_feat, motion], 1), "SeqConv")
        dflow = orc.xhead(sd, h, "flow_pred", "flow")
        mask = torch.sigmoid(orc.xhead(sd, h, "mask_pred", "mask"))
        dff = orc.conv_module(orc.conv_module(dflow, sd, "delta_flow_encoder.0", "ReLU", padding=3),
                              sd, "delta_flow_encoder.1", "ReLU", padding=1)
        mf = orc.conv_module(orc.conv_module(mask, sd, "mask_encoder.0", "ReLU", padding=1), sd,
                             "mask_encoder.1", "ReLU", padding=1)
        drot, dtr = orc.pose_head(sd, torch.cat([h, dff, mf], 1), label, 21)
        flow_pred = scale * orc.upsample(flow + dflow, scale)
        up_mask = orc.upsample(mask, scale)
        R, tr = orc.pose_update(drot, dtr, R.detach(), tr.detach(), depth_transform="exp",
                                detach_depth_for_xy=True)
        flow = orc.pose_flow(R, tr, K, points, valid, invalid_flow_num)
        for lst, v in zip(outs, (flow, flow_pred, R, tr, up_mask, drot, dtr)):
            lst.append(v)
    return outs


def test_masked_train_loop_restates_the_oracle_loop():
    """With the detach taken out of the picture (no autograd), the composition above is the
    oracle's masked decoder bit for bit."""
    inp = decoder_inputs(1, 256, seed=3)
    sd = oracle_state_dict()
    with torch.no_grad():
        a = orc.decoder_forward(sd, **inp, iters=3, mask_flow=True, mask_corr=True, train=True)
        b = masked_train_decoder_forward(sd, **inp, iters=3)
    for la, lb in zip(a, b):
        for x, y in zip(la, lb):
            assert torch.equal(x, y)


def test_oracle_masked_train_matches_reference_fixture(monkeypatch):
    """tests/test_train_golden.py's asserts on the masked training fixture (detach_mask=True, 3
    iterations): losses rtol 1e-4, all 149 gradient norms."""
    g = masked_train_fixture()
    B, S, iters, seed, *labels = (int(x) for x in g["meta"])
    monkeypatch.setattr(orc, "decoder_forward", masked_train_decoder_forward)
    batch, points, diam = train_batch(B, S, seed=seed, labels=labels, dtype=torch.float64)
    sd = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in refiner_state_dict().items()}
    loss, lp, lf, lm, outs, gt_flow = orc.refine_train_forward(
        sd, batch["render_images"], batch["real_images"], batch["ref_rotation"],
        batch["ref_translation"], batch["gt_rotation"], batch["gt_translation"], batch["depth"],
        batch["internel_k"], batch["label"], [p.double() for p in points], diam,
        gt_masks=batch["gt_masks"], iters=iters)
    loss.backward()
    np.testing.assert_allclose([loss.item(), lp.item(), lf.item(), lm.item()], g["losses"], rtol=1e-4)
    np.testing.assert_allclose(torch.stack(outs[2]).detach().numpy(), g["R"], atol=1e-5)
    np.testing.assert_allclose(torch.stack(outs[3]).detach().numpy(), g["t"], rtol=1e-5, atol=1e-3)
    names = [str(n) for n in g["grad_names"]]
    ref = dict(zip(names, g["grad_norms"]))
    dec_max = max(v for k, v in ref.items() if k.startswith("decoder.") and np.isfinite(v))
    enc_max = max(v for k, v in ref.items() if not k.startswith("decoder.") and np.isfinite(v))
    checked = 0
    for n in names:
        if n.startswith("encoder."):
            gs = [sd[p + n[len("encoder."):]].grad for p in ("real_encoder.", "render_encoder.")]
            gs = [x for x in gs if x is not None]
            o = float(sum(gs).norm()) if gs else float("nan")
        else:
            k = n[len("decoder."):] if n.startswith("decoder.") else n
            o = float("nan") if sd[k].grad is None else float(sd[k].grad.norm())
        r = ref[n]
        if not np.isfinite(r):
            assert not np.isfinite(o) or o == 0.0, n
            continue
        tol = 1e-3 * dec_max if n.startswith("decoder.") else 2e-2 * enc_max
        assert abs(o - r) <= tol + 1e-3 * r, f"{n}: oracle {o:.6e} vs reference {r:.6e}"
        checked += 1
    assert checked == len(names) == 149


def test_masking_is_separable_from_no_masking():
    """B=2, 256², seed 21, weight seed 1, 3 iterations: at iteration 2 every flag combination
    differs from the unmasked decoder by ≥ 5e-3 px per-sample mean EPE — 5× the 1e-3 px parity
    bar, so a parity test tells a masked decoder from an unmasked one."""
    inp = decoder_inputs(2, 256, seed=21)
    sd = oracle_state_dict(seed=1)
    with torch.no_grad():
        plain = orc.decoder_forward(sd, **inp, iters=3)
        for mf, mc in ((True, False), (False, True), (True, True)):
            out = orc.decoder_forward(sd, **inp, iters=3, mask_flow=mf, mask_corr=mc)
            epe = orc.cal_epe_mean(plain[0][2], out[0][2])
            print(f"mask_flow={mf} mask_corr={mc}: EPE vs unmasked {epe.tolist()}")
            assert float(epe.min()) >= 5e-3, (mf, mc, epe)


def test_lib_declares_the_masked_exports():
    from scflow_amd import _lib
    assert _lib.ABI_VERSION == 4
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "scflow_hip.h")).read()
    assert "#define SCFLOW_ABI_VERSION 4" in header
    for name in ("scflow_corr_lookup_masked", "scflow_corr_lookup_conv1x1_masked",
                 "scflow_pose_step_masked", "scflow_flow_downsample_masked",
                 "scflow_corr_lookup_backward_masked"):
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    lib = _lib.load()
    assert lib.scflow_abi_version() == 4
    # argument errors return codes without touching a device
    assert lib.scflow_corr_lookup_masked(None, None, 0, None, None, 0, 0, 1, 8, 8, 4, 4, 1, 0, None) == -1
    assert lib.scflow_corr_lookup_backward_masked(None, 0, 0, None, 0, None, None, 1, 8, 8, 4, 4, None) == -1


class _NoDevice:
    """Stands in for every tensor argument: any use is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"decoder_train touched an input ({name}) before checking its flags")


@pytest.mark.parametrize("flags", [(True, False), (False, True), (True, True)])
def test_train_rejects_mask_flags_without_detach_mask(flags):
    from types import SimpleNamespace
    from scflow_amd.train.model import check_train_flags, decoder_train
    dec = SimpleNamespace(detach_flow=True, detach_mask=False, mask_flow=flags[0], mask_corr=flags[1])
    x = _NoDevice()
    with pytest.raises(NotImplementedError, match="detach_mask"):
        decoder_train(dec, x, x, x, x, x, x, x, x, x, 3)
    dec.detach_mask = True
    check_train_flags(dec)  # supported
    dec.detach_flow = False
    with pytest.raises(NotImplementedError, match="detach_flow"):
        decoder_train(dec, x, x, x, x, x, x, x, x, x, 3)
