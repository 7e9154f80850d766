"""GPU: ``RAFTEncoder.bf16`` and the refiners' ``enc_bf16`` — the stride-1 3×3 convs of the wired
residual stages on the bf16 direct conv (SCFLOW_CONV_BF16_3X3N).

Yardstick (reference only): D, the distance between the fp32 oracle and the oracle whose
BasicBlock rounds what the device rounds (tests/enc_bf16_restatement.py).  The device is asserted
within 2·D + the fp32 path's tolerance of the FP32 oracle.  The factor 2: the
device rounds at slightly different fp32 values than the emulation — its InstanceNorm statistics
and Winograd-free accumulation order are not the oracle's — so a value near a bf16 tie can round
the other way: the device is another sample of a perturbation of D's size, not the same
perturbation.  D itself must be at least ten times the fp32 tolerance and the device further from
the fp32 oracle than that tolerance, so the test tells rounding from not rounding.  Every test
prints its figures (profiles/enc_bf16/gputest_figures.txt carries a run's)."""
import pytest
import torch

from tests import enc_bf16_restatement as er
from tests import gru_bf16_restatement as gr
from tests.test_gpu_encoder import build_encoder, build_refiner

orc = pytest.importorskip("oracle.scflow_oracle")
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("norm,seed,B,S", [("IN", 1, 2, 256), ("BN", 2, 2, 256), ("IN", 1, 1, 512)])
def test_encoder_within_twice_the_emulated_drift(norm, seed, B, S):
    x, ref, emu = er.encoder_pair(norm, seed, B, S)
    D = float((emu - ref).abs().max())
    bracket = 3e-4 + 1e-4 * float(ref.abs().max())  # test_encoder_matches_oracle's atol + rtol·max|ref|
    enc = build_encoder(norm, seed)
    xg = x.cuda()
    off0 = enc(xg)
    assert enc.last_bf16 == ()
    enc.bf16 = True
    try:
        on = enc(xg)
        assert enc.last_bf16 == er.wired_convs()
    finally:
        enc.bf16 = False
    off1 = enc(xg)
    torch.cuda.synchronize()
    assert enc.last_bf16 == ()
    assert torch.equal(off0, off1)  # the knob leaves no state behind
    d_ref, d_emu = float((on.cpu() - ref).abs().max()), float((on.cpu() - emu).abs().max())
    d_off = float((off0.cpu() - ref).abs().max())
    print(f"enc {norm} B={B} {S}²: D {D:.3e}  device-fp32 oracle {d_ref:.3e}  device-emulated oracle "
          f"{d_emu:.3e}  bound {2 * D + bracket:.3e}  fp32 tolerance {bracket:.3e}  "
          f"(knob off: {d_off:.3e})")
    assert torch.isfinite(on).all()
    assert D >= 10 * bracket, (D, bracket)
    assert d_ref <= 2 * D + bracket, (d_ref, D, bracket)
    assert d_ref > bracket, (d_ref, bracket)
    assert d_off <= bracket


def _get_pose(r, inp, iters):
    r.decoder.iters = iters
    g = {k: v.cuda() for k, v in inp.items()}
    out = r.get_pose(g["render_images"], g["real_images"], g["ref_rotation"], g["ref_translation"],
                     g["depth"], g["internel_k"], g["label"])
    torch.cuda.synchronize()
    return [[v.cpu() for v in lst] for lst in out]


def _check(tag, out, ref, emu):
    d_ref, d_dev, d_emu = gr.distances(emu, ref), gr.distances(out, ref), gr.distances(out, emu)
    tol = gr.granted(ref)
    for f in gr.FAMILIES:
        print(f"{tag} {f}: D_ref {d_ref[f]:.3e}  device-fp32 oracle {d_dev[f]:.3e}  "
              f"device-emulated oracle {d_emu[f]:.3e}  bound {2 * d_ref[f] + tol[f]:.3e}  "
              f"fp32 tolerance {tol[f]:.3e}")
    for lst in out:
        assert all(torch.isfinite(v).all() for v in lst)
    for f in gr.FAMILIES:
        assert d_dev[f] <= 2 * d_ref[f] + tol[f], (tag, f, d_dev[f], d_ref[f], tol[f])


@pytest.mark.parametrize("knobs", ["enc_bf16", "all three"])
def test_refiner_get_pose_within_twice_the_emulated_drift(knobs):
    """get_pose on the refine golden's inputs (B = 2, 256², 4 iterations) with ``enc_bf16`` alone
    and with ``decoder.gru_bf16`` and ``decoder.menc_bf16`` too, against the oracle emulating the
    same knobs."""
    inp, iters, ref, emu_enc, emu_all = er.refine_pair()
    r = build_refiner()
    both = knobs == "all three"
    r.enc_bf16, r.decoder.gru_bf16, r.decoder.menc_bf16 = True, both, both
    out = _get_pose(r, inp, iters)
    assert r.real_encoder.last_bf16 == r.context.last_bf16 == er.wired_convs()
    assert bool(r.decoder.last_plan.get("gru_bf16")) is both
    assert bool(r.decoder.last_plan.get("menc_bf16")) is both
    _check(knobs, out, ref, emu_all if both else emu_enc)
    r.enc_bf16 = r.decoder.gru_bf16 = r.decoder.menc_bf16 = False
    off = _get_pose(r, inp, iters)
    assert r.real_encoder.last_bf16 == r.context.last_bf16 == ()
    d_off, tol = gr.distances(off, ref), gr.granted(ref)
    assert all(d_off[f] <= tol[f] for f in gr.FAMILIES), d_off


def test_extract_feat_takes_the_knob():
    inp, _, _, _, _ = er.refine_pair()
    r = build_refiner()
    args = inp["render_images"].cuda(), inp["real_images"].cuda()
    off0 = r.extract_feat(*args)
    r.enc_bf16 = True
    on = r.extract_feat(*args)
    assert r.real_encoder.last_bf16 == r.context.last_bf16 == er.wired_convs()
    r.enc_bf16 = False
    off1 = r.extract_feat(*args)
    torch.cuda.synchronize()
    assert r.real_encoder.last_bf16 == r.context.last_bf16 == ()
    assert all(torch.equal(a, b) for a, b in zip(off0, off1))
    if er.WIRED:
        assert all(not torch.equal(a, b) for a, b in zip(off0, on))


def test_uncovered_map_raises():
    """A 128² image: the third stage's maps are 16 wide, outside the kernel's domain.  With the
    knob on and that stage wired the forward raises ScflowError — nothing falls back to fp32; off
    it runs, and off again it gives the first result bit for bit."""
    from scflow_amd import synthetic
    from scflow_amd._lib import ScflowError
    from tests.helpers import t
    x = t(synthetic.make_images(1, 128, seed=3)["real_images"]).cuda()
    for norm, seed in (("IN", 1), ("BN", 2)):
        enc = build_encoder(norm, seed)
        off0 = enc(x)
        enc.bf16 = True
        try:
            if "res_layer3" in er.WIRED:
                with pytest.raises(ScflowError):
                    enc(x)
            else:
                assert torch.isfinite(enc(x)).all()
        finally:
            enc.bf16 = False
        assert torch.equal(enc(x), off0) and enc.last_bf16 == ()
    torch.cuda.synchronize()
