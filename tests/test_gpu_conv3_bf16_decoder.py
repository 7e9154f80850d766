"""GPU: the decoders with ``menc_bf16 = True`` — the motion encoder's 3×3 convs (corr_net.1,
flow_net.1, out_net) on the bf16 direct 3×3 kernel — alone and together with ``gru_bf16``.

Yardstick (reference only; tests/test_gpu_gru_bf16_decoder.py's, unchanged): D_ref, the distance
per output family between the fp32 oracle and the oracle whose MotionEncoder (and, for both knobs,
ConvGRU) rounds what the device rounds (tests/conv3_bf16_restatement.py).  The device is asserted
within 2·D_ref + the fp32 path's tolerance of the FP32 oracle.  The factor 2: the device rounds at
slightly different fp32 values than the emulation, so a value near a bf16 tie can round the other
way — its trajectory is another sample of a perturbation of D_ref's size, not the same
perturbation.  Each test prints D_ref, the device's distance to the fp32 oracle and to the emulated
oracle (DESIGN.md §25 and profiles/menc_bf16/gputest_figures.txt carry a run's figures)."""
import pytest
import torch

from tests import conv3_bf16_restatement as cr
from tests import gru_bf16_restatement as gr
from tests import raft_restatement as rr
from tests.helpers import decoder_inputs
from tests.test_gpu_decoder import build_decoder, run_gpu

orc = pytest.importorskip("oracle.scflow_oracle")
pytestmark = pytest.mark.gpu

CASE = (2, 256, 31, 4, 5)  # B, S, input seed, iterations, weight seed (test_conv3_bf16_host's too)


def check(tag, out, ref, emu):
    d_ref, d_dev, d_emu = gr.distances(emu, ref), gr.distances(out, ref), gr.distances(out, emu)
    tol = gr.granted(ref)
    for f in gr.FAMILIES:
        print(f"{tag} {f}: D_ref {d_ref[f]:.3e}  device-fp32 oracle {d_dev[f]:.3e}  "
              f"device-emulated oracle {d_emu[f]:.3e}  bound {2 * d_ref[f] + tol[f]:.3e}")
    for lst in out:
        assert all(torch.isfinite(v).all() for v in lst)
    for f in gr.FAMILIES:
        assert d_dev[f] <= 2 * d_ref[f] + tol[f], (tag, f, d_dev[f], d_ref[f], tol[f])


def run_knobs(dec, inp, gru=False):
    dec.menc_bf16, dec.gru_bf16 = True, gru
    try:
        return run_gpu(dec, inp), dec.last_plan
    finally:
        dec.menc_bf16 = dec.gru_bf16 = False


def test_decoder_within_twice_the_reference_drift():
    inp, dec, ref, emu = cr.oracle_pair(*CASE)
    out, plan = run_knobs(dec, inp)
    assert plan["menc_bf16"] is True and "gru_bf16" not in plan
    check("menc", out, ref, emu)


def test_decoder_with_both_knobs():
    """menc_bf16 and gru_bf16 together, against the oracle that emulates both roundings."""
    inp, dec, ref, emu = cr.oracle_pair(*CASE, True)
    out, plan = run_knobs(dec, inp, gru=True)
    assert plan["menc_bf16"] is True and plan["gru_bf16"] is True
    check("menc+gru", out, ref, emu)


def test_plan_key_and_toggling_leave_no_state():
    inp, dec, _, _ = cr.oracle_pair(*CASE)
    off0 = run_gpu(dec, inp)
    plan_off = dec.last_plan
    assert "menc_bf16" not in plan_off
    on, plan = run_knobs(dec, inp)
    # the knob adds its key and changes nothing else of the schedule
    assert plan == dict(plan_off, menc_bf16=True)
    dec.gru_bf16 = True  # the other knob alone does not set this one's key
    try:
        run_gpu(dec, inp)
        assert dec.last_plan.get("gru_bf16") is True and "menc_bf16" not in dec.last_plan
    finally:
        dec.gru_bf16 = False
    off1 = run_gpu(dec, inp)
    assert "menc_bf16" not in dec.last_plan and "gru_bf16" not in dec.last_plan
    for a, b in zip(off0, off1):
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    assert any(not torch.equal(u, v) for a, b in zip(off0, on) for u, v in zip(a, b))


def test_decoder_512_feat64():
    """64×64 feature maps (two column blocks per row block), B = 1, 2 iterations."""
    inp, dec, ref, emu = cr.oracle_pair(1, 512, 5, 2, 2, False, (64, 64))
    out, plan = run_knobs(dec, inp)
    assert plan["menc_bf16"] is True
    check("512", out, ref, emu)


def test_raft_decoder():
    """RAFTDecoder takes the knob through the shared core.  Families: the last upsampled flow's
    mean EPE and the low-resolution flows, at tests/test_gpu_raft_decoder.py's tolerances."""
    inp = rr.raft_inputs(2, 256, seed=23)
    dec = rr.build_raft_decoder("RAFTDecoder", 4, seed=3)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = rr.raft_forward(sd, **inp, iters=4, occlusion=False)
    with cr.emulating():
        emu = rr.raft_forward(sd, **inp, iters=4, occlusion=False)
    dec.menc_bf16, dec.keep_lr_flows = True, True
    up = [x.cpu() for x in dec.cuda()(**{k: v.cuda() for k, v in inp.items()})]
    torch.cuda.synchronize()
    lr = torch.stack([x.cpu() for x in dec.lr_flows])
    assert dec.last_plan == dict(convex=True, fuse_lc=True, tiled=True, hoist=True, menc_bf16=True)

    def dist(a_up, a_lr, b_up, b_lr):
        return dict(epe=rr.mean_epe(b_up, a_up), lr=float((a_lr - b_lr).abs().max()))
    r_lr, e_lr = torch.stack(ref["lr_flow"]), torch.stack(emu["lr_flow"])
    d_ref = dist(emu["upflow"][-1], e_lr, ref["upflow"][-1], r_lr)
    d_dev = dist(up[-1], lr, ref["upflow"][-1], r_lr)
    d_emu = dist(up[-1], lr, emu["upflow"][-1], e_lr)
    tol = dict(epe=rr.EPE_TOL, lr=1e-3)
    for f in ("epe", "lr"):
        print(f"raft {f}: D_ref {d_ref[f]:.3e}  device-fp32 restatement {d_dev[f]:.3e}  "
              f"device-emulated {d_emu[f]:.3e}  bound {2 * d_ref[f] + tol[f]:.3e}")
    for f in ("epe", "lr"):
        assert d_ref[f] > 0 and d_dev[f] <= 2 * d_ref[f] + tol[f], (f, d_dev[f], d_ref[f])
    dec.menc_bf16 = False
    dec.cuda()(**{k: v.cuda() for k, v in inp.items()})
    assert "menc_bf16" not in dec.last_plan


def test_uncovered_feature_size_raises():
    """A feature map outside the kernel's domain raises ScflowError; nothing falls back to fp32.

    Through the decoder: 48×48 maps (384² patches) with the knob on.  (Square maps the fp32
    decoder runs are 32 or 64 wide, which the bf16 kernel covers too: at 48 the fp32 GRU convs are
    refused as well, so this half only pins that the knob does not turn a refusal into a run.)
    Through the module, where the bf16 domain is the narrower one: a 6×64 map, which every fp32
    kernel of the motion encoder takes (F(2×2,3×3) needs whole pairs of rows at W = 64, the bf16
    kernel whole 4-row blocks) — off it runs, on it is refused by scflow_conv2d
    (SCFLOW_EUNSUPPORTED), off again it gives the first result bit for bit."""
    from scflow_amd._lib import ScflowError
    inp = decoder_inputs(1, 384, seed=2)
    dec = build_decoder(1, feat_size=(48, 48))
    dec.menc_bf16 = True
    try:
        with pytest.raises(ScflowError):
            run_gpu(dec, inp)
    finally:
        dec.menc_bf16 = False

    enc = build_decoder(1).encoder.cuda()
    g = torch.Generator().manual_seed(4)
    corr = torch.randn(1, 324, 6, 64, generator=g).cuda()
    flow = torch.randn(1, 2, 6, 64, generator=g).cuda()
    with torch.no_grad():
        off0 = enc(corr, flow)
        assert off0.shape == (1, 128, 6, 64) and torch.isfinite(off0).all()
        enc.bf16 = True
        try:
            with pytest.raises(ScflowError, match="scflow_conv2d failed with code -2"):
                enc(corr, flow)
        finally:
            enc.bf16 = False
        assert torch.equal(enc(corr, flow), off0)
    torch.cuda.synchronize()
