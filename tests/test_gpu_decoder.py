"""GPU parity of the whole SCFlowDecoder forward (the drop-in boundary) vs the reference.

Bar (BASELINE.json north_star): flow endpoint error within 1e-3 px of the reference, fp32.
* golden fixture produced by the reference itself (B=2, 256², 4 iterations);
* the CPU oracle (pinned to the reference) at B=4 / 8 iterations and at 512² (pose head
  feat_size=(64,64));
* poses: rotations within 1e-5, translations within 1e-3 mm.
"""
import numpy as np
import pytest
import torch

from tests.helpers import decoder_inputs, golden, t

orc = pytest.importorskip("oracle.scflow_oracle")

EPE_TOL = 1e-3  # px, mean EPE per sample (cal_epe 'mean', models/utils/flow.py:64-78)


def decoder_cfg(iters=4, feat_size=None, rotation_mode="ortho6d"):
    """The decoder block of configs/refine_models/scflow_ycbv_real.py:207-230."""
    from scflow_amd.modules import MultiClassPoseHead
    head = dict(type=MultiClassPoseHead, num_class=21, in_channels=224, net_type="Basic",
                rotation_mode=rotation_mode, norm_cfg=dict(type="GN", num_groups=32, requires_grad=True),
                act_cfg=dict(type="ReLU"))
    if feat_size is not None:
        head["feat_size"] = feat_size
    return dict(net_type="Basic", num_levels=4, radius=4, iters=iters, detach_flow=True,
                detach_mask=True, detach_pose=True, detach_depth_for_xy=True, mask_flow=False,
                mask_corr=False, pose_head_cfg=head, corr_lookup_cfg=dict(align_corners=True),
                gru_type="SeqConv", act_cfg=dict(type="ReLU"))


def build_decoder(iters=4, feat_size=None, seed=0, rotation_mode="ortho6d"):
    from scflow_amd import MODELS, synthetic
    from scflow_amd.decoder import SCFlowDecoder
    dec = MODELS.build(dict(type="SCFlowDecoder", **decoder_cfg(iters, feat_size, rotation_mode)))
    assert isinstance(dec, SCFlowDecoder)
    synthetic.fill_module_(dec, seed=seed)
    return dec.eval()


def run_gpu(dec, inp):
    gi = {k: v.cuda() for k, v in inp.items()}
    out = dec.cuda()(**gi, invalid_flow_num=0.0)
    torch.cuda.synchronize()
    return [[x.cpu() for x in lst] for lst in out]


def check_against(out, ref_flow_pose, ref_flow_pred, ref_R=None, ref_t=None):
    epe_pose = orc.cal_epe_mean(ref_flow_pose, out[0][-1])
    epe_pred = orc.cal_epe_mean(ref_flow_pred, out[1][-1])
    assert float(epe_pose.max()) <= EPE_TOL, f"pose-flow EPE {epe_pose}"
    assert float(epe_pred.max()) <= EPE_TOL, f"pred-flow EPE {epe_pred}"
    if ref_R is not None:
        np.testing.assert_allclose(torch.stack(out[2]).numpy(), ref_R, atol=1e-5)
        np.testing.assert_allclose(torch.stack(out[3]).numpy(), ref_t, rtol=1e-6, atol=1e-3)
    return float(epe_pose.max()), float(epe_pred.max())


@pytest.mark.gpu
def test_decoder_matches_reference_golden():
    g = golden("e2e")
    B, S, iters, seed = (int(v) for v in g["meta"])
    inp = decoder_inputs(B, S, seed, g)
    out = run_gpu(build_decoder(iters), inp)
    assert len(out) == 7 and all(len(l) == iters for l in out)
    check_against(out, t(g["flow_pose_last"]), t(g["flow_pred_last"]), g["R"], g["t"])
    np.testing.assert_allclose(torch.stack(out[5]).numpy(), g["drot"], atol=1e-5)
    np.testing.assert_allclose(torch.stack(out[6]).numpy(), g["dt"], atol=1e-5)
    np.testing.assert_allclose(out[4][-1].numpy(), g["mask_last"], atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("hoist", [True, False])
def test_decoder_matches_oracle_b4_8iters(hoist):
    """hoist: the context's GRU contribution computed once per forward (default) or the
    reference's full-width GRU convs every iteration."""
    inp = decoder_inputs(4, 256, seed=21)
    dec = build_decoder(8, seed=1)
    dec.hoist_context = hoist
    out = run_gpu(dec, inp)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = orc.decoder_forward(sd, **inp, iters=8)
    check_against(out, ref[0][-1], ref[1][-1], torch.stack(ref[2]).numpy(), torch.stack(ref[3]).numpy())
    # every iteration, not just the last
    for i in range(8):
        assert float(orc.cal_epe_mean(ref[0][i], out[0][i]).max()) <= EPE_TOL


@pytest.mark.gpu
def test_decoder_unfused_xhead_matches_oracle():
    """The XHead predictors as separate launches (fuse_xhead_pred = False; the default fuses them
    into the hidden conv, covered by the other decoder tests) — a different fp32 summation order,
    so against the oracle, every iteration."""
    inp = decoder_inputs(4, 256, seed=29)
    dec = build_decoder(4, seed=2)
    dec.fuse_xhead_pred = False
    out = run_gpu(dec, inp)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = orc.decoder_forward(sd, **inp, iters=4)
    check_against(out, ref[0][-1], ref[1][-1], torch.stack(ref[2]).numpy(), torch.stack(ref[3]).numpy())
    for i in range(4):
        assert float(orc.cal_epe_mean(ref[0][i], out[0][i]).max()) <= EPE_TOL


@pytest.mark.gpu
def test_decoder_schedules_bit_identical():
    """The launch schedule does not change the arithmetic: the fused iteration tail
    (scflow_pose_step, double-buffered ↓8 flow) vs separate launches, the side stream vs one
    stream, device-scope vs default events, the tail branches paired (scflow_conv2d_pair) vs on
    two streams give bit-identical outputs (every one of the 7 lists, every iteration)."""
    inp = decoder_inputs(2, 256, seed=13)
    dec = build_decoder(3, seed=4)
    base = run_gpu(dec, inp)
    for fuse, side, dse, pair in ((False, True, True, 1), (True, False, True, 1),
                                  (False, False, True, 1), (True, True, False, 1),
                                  (True, True, True, 0), (False, True, True, 0)):
        dec.fuse_tail, dec.side_stream, dec.device_scope_events = fuse, side, dse
        dec.pair_tail = pair  # round 6: the tail's two branches paired on one stream, or two streams
        out = run_gpu(dec, inp)
        for a, b in zip(base, out):
            for x, y in zip(a, b):
                assert torch.equal(x, y), (fuse, side, dse, pair)
    dec.fuse_tail, dec.side_stream, dec.device_scope_events, dec.pair_tail = True, True, True, -1


@pytest.mark.gpu
def test_decoder_pingpong_halves_equal_whole_batch():
    """_forward_pingpong (two interleaved halves on two stream pairs, both taking the whole
    batch's label[0] for the pose head) against the single-schedule forward of the same
    multi-class batch: every list, every iteration.  Not bit-identical — a half-batch launch may
    pick other K splits (pose-head GroupNorm partials) — so EPE ≤ 1e-4 px and rotations /
    translations to fp32 rounding."""
    inp = decoder_inputs(8, 256, seed=17)
    inp["label"] = torch.tensor([3, 11, 0, 7, 20, 3, 15, 9])
    dec = build_decoder(4, seed=8)
    dec.pingpong = False
    whole = run_gpu(dec, inp)
    dec.pingpong, dec.pingpong_min = True, 4
    halves = run_gpu(dec, inp)
    for k in (0, 1):
        for a, b in zip(whole[k], halves[k]):
            assert float(orc.cal_epe_mean(a, b).max()) <= 1e-4
    for k in (2, 3, 5, 6):
        for a, b in zip(whole[k], halves[k]):
            torch.testing.assert_close(b, a, rtol=1e-5, atol=1e-5)
    for a, b in zip(whole[4], halves[4]):
        torch.testing.assert_close(b, a, rtol=0, atol=1e-5)


@pytest.mark.gpu
def test_decoder_quaternion_rotation_mode():
    """rotation_mode='quaternion' (pose_head.py:175-176, pose.py:132-133): the pose head emits
    4 values per class and the pose kernels apply a quaternion ΔR (x, y, z, w — see the oracle's
    rotation_from_quaternion_xyzw; kornia itself is absent, so this branch is parity unpinned
    against the reference and checked against the oracle restatement only)."""
    inp = decoder_inputs(2, 256, seed=19)
    dec = build_decoder(3, seed=9, rotation_mode="quaternion")
    out = run_gpu(dec, inp)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = orc.decoder_forward(sd, **inp, iters=3)
    assert out[5][0].shape == (2, 4)
    for i in range(3):
        assert float(orc.cal_epe_mean(ref[0][i], out[0][i]).max()) <= EPE_TOL
        assert float(orc.cal_epe_mean(ref[1][i], out[1][i]).max()) <= EPE_TOL
        np.testing.assert_allclose(out[2][i].numpy(), ref[2][i].numpy(), atol=1e-5)
        np.testing.assert_allclose(out[3][i].numpy(), ref[3][i].numpy(), rtol=1e-6, atol=1e-3)


@pytest.mark.gpu
def test_decoder_512_feat64():
    inp = decoder_inputs(1, 512, seed=5)
    dec = build_decoder(2, feat_size=(64, 64), seed=2)
    out = run_gpu(dec, inp)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = orc.decoder_forward(sd, **inp, iters=2)
    check_against(out, ref[0][-1], ref[1][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
def test_decoder_odd_batch_matches_oracle(B):
    """Batch sizes at which the pose head's gather conv has a ragged pixel tile (B = 1: M = 16,
    half a tile; B = 3: M = 48) and its GroupNorm reduce other slab counts than at B = 2, 4, 8."""
    inp = decoder_inputs(B, 256, seed=33 + B)
    dec = build_decoder(2, seed=3)
    out = run_gpu(dec, inp)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = orc.decoder_forward(sd, **inp, iters=2)
    check_against(out, ref[0][-1], ref[1][-1], torch.stack(ref[2]).numpy(), torch.stack(ref[3]).numpy())


@pytest.mark.gpu
def test_decoder_iters_attribute_is_reread():
    inp = decoder_inputs(1, 256, seed=2)
    dec = build_decoder(4)
    dec.iters = 2
    out = run_gpu(dec, inp)
    assert all(len(l) == 2 for l in out)


def test_decoder_rejects_cpu_inputs():
    from scflow_amd._lib import ScflowError
    inp = decoder_inputs(1, 64, seed=2)
    dec = build_decoder(1)
    with pytest.raises(ScflowError):
        dec(**inp, invalid_flow_num=0.0)
