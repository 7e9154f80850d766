"""GPU: the decoders with ``gru_bf16 = True`` — the GRU's z|r and q convs on the bf16 direct kernel.

Yardstick (reference only): D_ref, the distance per output family between the fp32 oracle and the
oracle whose ConvGRU rounds what the device rounds (tests/gru_bf16_restatement.py).  The device is
asserted within 2·D_ref + the fp32 path's tolerance of the FP32 oracle.  The factor 2: the device
rounds at slightly different fp32 values than the emulation, so a value near a bf16 tie can round
the other way — its trajectory is another sample of a perturbation of D_ref's size, not the same
perturbation.  Each test prints D_ref, the device's distance to the fp32 oracle and to the emulated
oracle (DESIGN.md §bf16 GRU convs and profiles/gru_bf16/gputest_figures.txt carry a run's figures).

Graph capture of the bf16 path is out of scope: its launches are ordinary kernel launches."""
import pytest
import torch

from tests import gru_bf16_restatement as gr
from tests import raft_restatement as rr
from tests.test_gpu_decoder import run_gpu

orc = pytest.importorskip("oracle.scflow_oracle")
pytestmark = pytest.mark.gpu

CASE = (2, 256, 31, 4, 5)  # B, S, input seed, iterations, weight seed (test_gru_bf16_host's too)


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


def run_bf16(dec, inp, **knobs):
    dec.gru_bf16 = True
    for k, v in knobs.items():
        setattr(dec, k, v)
    try:
        return run_gpu(dec, inp), dec.last_plan
    finally:
        dec.gru_bf16 = False
        dec.hoist_context = True


def test_decoder_within_twice_the_reference_drift():
    inp, dec, ref, emu = gr.oracle_pair(*CASE, 128)
    out, plan = run_bf16(dec, inp)
    assert plan["gru_bf16"] is True
    check("hoisted", out, ref, emu)


def test_decoder_full_width_gru():
    """hoist_context = False: the context channels go through the bf16 convs too (c0 = 384 for
    z|r, 128 + 256 for q); the emulation then rounds everything (cxt_channels = 0)."""
    inp, dec, ref, emu = gr.oracle_pair(*CASE, 0)
    out, plan = run_bf16(dec, inp, hoist_context=False)
    assert plan["gru_bf16"] is True
    check("full width", out, ref, emu)


def test_plan_key_and_toggling_leave_no_state():
    inp, dec, _, _ = gr.oracle_pair(*CASE, 128)
    off0 = run_gpu(dec, inp)
    assert "gru_bf16" not in dec.last_plan
    on, plan = run_bf16(dec, inp)
    assert plan["gru_bf16"] is True and {k: v for k, v in plan.items() if k != "gru_bf16"} == \
        {k: v for k, v in dec.last_plan.items() if k != "gru_bf16"}
    off1 = run_gpu(dec, inp)
    assert "gru_bf16" not in dec.last_plan
    for a, b in zip(off0, off1):
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    assert any(not torch.equal(u, v) for a, b in zip(off0, on) for u, v in zip(a, b))


def test_decoder_512_feat64():
    """64×64 feature maps (W = 64: two rows per 1×5 workgroup, two column blocks per 5×1 row
    block), B = 1, 2 iterations."""
    inp, dec, ref, emu = gr.oracle_pair(1, 512, 5, 2, 2, 128, (64, 64))
    out, plan = run_bf16(dec, inp)
    assert plan["gru_bf16"] is True
    check("512", out, ref, emu)


def test_raft_decoder(monkeypatch):
    """RAFTDecoder takes the knob through the shared core.  Families: the last upsampled flow's
    mean EPE and the low-resolution flows, at tests/test_gpu_raft_decoder.py's tolerances."""
    inp = rr.raft_inputs(2, 256, seed=23)
    dec = rr.build_raft_decoder("RAFTDecoder", 4, seed=3)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = rr.raft_forward(sd, **inp, iters=4, occlusion=False)
    monkeypatch.setattr(orc, "conv_gru", gr.emulated(128))
    emu = rr.raft_forward(sd, **inp, iters=4, occlusion=False)
    monkeypatch.undo()
    dec.gru_bf16, dec.keep_lr_flows = True, True
    up = [x.cpu() for x in dec.cuda()(**{k: v.cuda() for k, v in inp.items()})]
    torch.cuda.synchronize()
    lr = torch.stack([x.cpu() for x in dec.lr_flows])
    assert dec.last_plan == dict(convex=True, fuse_lc=True, tiled=True, hoist=True, gru_bf16=True)

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
    dec.gru_bf16 = False
    dec.cuda()(**{k: v.cuda() for k, v in inp.items()})
    assert "gru_bf16" not in dec.last_plan

