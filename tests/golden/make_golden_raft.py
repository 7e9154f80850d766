"""Fixtures of the RAFT baseline decoders from the REFERENCE's own modules
(``models/decoder/raft_decoder_mask.py`` RAFTDecoderMask, ``models/decoder/raft_decoder.py``
RAFTDecoder), with ``make_golden``'s shims and stand-ins and ``scflow_amd.synthetic``'s inputs and
weights.

    python tests/golden/make_golden_raft.py

writes
* ``golden_raft_b2_s256_it4.npz``: the last ``upocclusion`` of RAFTDecoderMask, the low-resolution
  flow after every iteration, checksums of the regenerated inputs, the state-dict key names and
  shapes of both reference modules, the gain (below) and the two refusal figures;
* ``golden_raft_b2_s256_it4_upflow.npz``: the last ``upflow`` — 1 MiB of floats on its own, kept
  in a file of its own so that no fixture exceeds the repository's 1 MiB limit.

Inputs (``make_decoder_inputs(B, S, seed)``: feat_render → feat1, feat_real → feat2, zero flow at
the feature resolution) and weights (``fill_module_(decoder, seed)``) are regenerated from the
seeds by the tests; only outputs are stored.  RAFTDecoder is run with the same seed: its
parameters are RAFTDecoderMask's without the occlusion head, so its ``upflow`` must equal the mask
decoder's bit for bit — the generator asserts that, and the tests compare both against one array.

``fill_module_``'s unit-variance weights give mask logits whose scaled softmax is nearly uniform,
and a uniform softmax would hide a wrong channel order.  ``mask_pred.predict_layer.weight`` is
therefore multiplied by ``GAIN`` (a power of two: exact in every precision; stored in the fixture,
applied by the tests).

The generator refuses to write unless
1. in every iteration at least half of the (pixel, sub-pixel) softmaxes have their largest weight
   inside (0.2, 0.9), and
2. the mean endpoint error between the float32 and the float64 run's last ``upflow`` is at most
   1e-4 px (a tenth of the project's 1e-3 px gate): otherwise the recurrence at these weights is
   too ill-conditioned for the gate to mean anything.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from scflow_amd import synthetic  # noqa: E402

NAME = "golden_raft_b2_s256_it4"
B, S, ITERS, IN_SEED, W_SEED = 2, 256, 4, 11, 0
GAIN = 32.0
FLAT_BOUNDS, FLAT_MIN_FRACTION = (0.2, 0.9), 0.5
COND_MAX_EPE = 1e-4


def raft_decoder_cfg(iters=ITERS):
    """The decoder block of configs/refine_models/raft.py:40-48 (without its `type`)."""
    return dict(net_type="Basic", num_levels=4, radius=4, iters=iters,
                corr_lookup_cfg=dict(align_corners=True), gru_type="SeqConv",
                act_cfg=dict(type="ReLU"))


def load_raft(ref):
    """make_golden.load_reference() loads raft_decoder.py; the mask decoder is a file of its own."""
    ref.raft_mask = mg._load("models.decoder.raft_decoder_mask", "models/decoder/raft_decoder_mask.py")
    return ref


def build(cls, dtype=torch.float32):
    dec = cls(**raft_decoder_cfg())
    synthetic.fill_module_(dec, seed=W_SEED)
    with torch.no_grad():
        dec.mask_pred.predict_layer.weight.mul_(GAIN)
    return dec.to(dtype).eval()


def run(dec, inputs, dtype=torch.float32):
    """→ (decoder output, low-resolution flow after every iteration, scaled logits per iteration)."""
    lr_flows, logits = [], []
    name = "upsample_flow" if hasattr(dec, "upsample_flow") else "_upsample"
    orig = getattr(dec, name)

    def watch(flow, mask=None):
        lr_flows.append(flow.detach().clone())
        logits.append(mask.detach().clone())
        return orig(flow, mask)
    setattr(dec, name, watch)
    t = {k: mg.t32(inputs[k]).to(dtype) for k in ("feat_render", "feat_real", "h_feat", "cxt_feat")}
    h, w = t["feat_render"].shape[-2:]
    # the reference casts the lookup (and its pixel grid) with `.float()` (corr_lookup.py:136): in
    # the float64 run that cast keeps the run's precision instead
    to_float = torch.Tensor.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        with torch.no_grad():
            out = dec(t["feat_render"], t["feat_real"], torch.zeros(B, 2, h, w, dtype=dtype),
                      t["h_feat"], t["cxt_feat"])
    finally:
        torch.Tensor.float = to_float
    return out, lr_flows, logits


def flat_fraction(scaled_logits):
    """Share of the (pixel, sub-pixel) softmaxes whose largest weight lies inside FLAT_BOUNDS."""
    n, _, h, w = scaled_logits.shape
    top = torch.softmax(scaled_logits.view(n, 9, 64, h, w), dim=1).amax(dim=1)
    return float(((top > FLAT_BOUNDS[0]) & (top < FLAT_BOUNDS[1])).double().mean())


def mean_epe(a, b):
    return float((a.double() - b.double()).pow(2).sum(1).sqrt().mean())


def save(name, out):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{name}.npz: {size} bytes")
    assert size <= 1 << 20, f"{name}.npz is larger than 1 MiB"


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref = load_raft(mg.load_reference())
    inputs = synthetic.make_decoder_inputs(B, S, seed=IN_SEED)
    dec = build(ref.raft_mask.RAFTDecoderMask)
    (upflow, upocc), lr_flows, logits = run(dec, inputs)
    assert len(upflow) == len(upocc) == len(lr_flows) == ITERS

    # refusal 1: a flat softmax would not tell a wrong channel order from the right one
    fracs = [flat_fraction(m) for m in logits]
    print("softmax: share of largest weights inside", FLAT_BOUNDS, "per iteration:",
          [f"{f:.3f}" for f in fracs], f"(need > {FLAT_MIN_FRACTION})")
    assert min(fracs) >= FLAT_MIN_FRACTION, f"flat or saturated softmax: {fracs}; change GAIN"

    # refusal 2: conditioning of the recurrence at these weights
    (upflow64, upocc64), _, _ = run(build(ref.raft_mask.RAFTDecoderMask, torch.float64), inputs,
                                    torch.float64)
    cond = mean_epe(upflow[-1], upflow64[-1])
    print(f"float32 vs float64 last upflow: mean EPE {cond:.3e} px (need <= {COND_MAX_EPE:.0e}); "
          f"upocclusion max |diff| {float((upocc[-1].double() - upocc64[-1]).abs().max()):.3e}")
    assert cond <= COND_MAX_EPE, f"ill-conditioned recurrence: mean EPE {cond}; change the seeds"

    # RAFTDecoder at the same seed: the same flow without the occlusion head
    plain = build(ref.raft.RAFTDecoder)
    upflow_p, lr_p, _ = run(plain, inputs)
    assert all(torch.equal(a, b) for a, b in zip(upflow, upflow_p)), "RAFTDecoder ≠ RAFTDecoderMask"
    assert all(torch.equal(a, b) for a, b in zip(lr_flows, lr_p))

    out = {}
    for k in ("feat_render", "feat_real", "h_feat", "cxt_feat"):
        out[f"sum_{k}"] = np.array([inputs[k].astype(np.float64).sum(),
                                    np.abs(inputs[k]).astype(np.float64).sum()])
    out["upocclusion_last"] = upocc[-1].numpy()
    out["lr_flow"] = torch.stack(lr_flows).numpy()
    out["upflow_absmean"] = np.array([f.abs().double().mean().item() for f in upflow])
    out["meta"] = np.array([B, S, ITERS, IN_SEED, W_SEED])
    out["gain"] = np.array(GAIN)
    out["flat_fraction"] = np.array(fracs)
    out["cond_mean_epe"] = np.array(cond)
    for tag, d in (("mask", dec), ("plain", plain)):
        sd = d.state_dict()
        out[f"state_keys_{tag}"] = np.array(list(sd.keys()))
        out[f"state_shapes_{tag}"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    save(NAME + "_upflow", {"upflow_last": upflow[-1].numpy()})
    save(NAME, out)
    print("upflow |mean| per iteration:", out["upflow_absmean"],
          " lr flow |max|:", float(np.abs(out["lr_flow"]).max()))


if __name__ == "__main__":
    main()
