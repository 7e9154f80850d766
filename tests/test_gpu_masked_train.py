"""GPU: training with occlusion masking (mask_flow = mask_corr = True, detach_mask = True) — the
HIP forward + backward against the fixture generated from the REFERENCE's own modules and losses
(tests/golden/make_golden_masked.py: 3 iterations, so a predicted mask crosses a detach and is
used twice), and two optimizer steps (loss decreases, bitwise reproducible)."""
import numpy as np
import pytest
import torch

from tests.test_masked_host import masked_train_fixture
from tests.test_train_host import build_train_refiner, train_batch

pytestmark = pytest.mark.gpu


def masked_refiner(iters):
    r = build_train_refiner(iters)
    r.decoder.mask_flow = r.decoder.mask_corr = True
    assert r.decoder.detach_mask is True
    return r.cuda()


def test_masked_train_forward_backward_matches_reference_fixture():
    """test_train_forward_backward_matches_reference_fixture's asserts and tolerances: losses
    rtol 1e-4, R 1e-5, every one of the 149 per-parameter gradient norms within 1e-3 of the
    decoder's largest norm (+1e-3 relative) / 2e-2 of the encoders'."""
    from scflow_amd.train.model import refiner_train_forward
    g = masked_train_fixture()
    B, S, iters, seed, *labels = (int(x) for x in g["meta"])
    assert iters == 3
    r = masked_refiner(iters)
    batch, points, diam = train_batch(B, S, seed=seed, labels=labels)
    gb = {k: v.cuda() for k, v in batch.items()}
    res = refiner_train_forward(r, gb, [p.cuda() for p in points], diam)
    res["loss"].backward()
    torch.cuda.synchronize()
    got = [res["loss"].item(), res["loss_pose"].item(), res["loss_flow"].item(), res["loss_mask"].item()]
    print("losses", got, "fixture", g["losses"].tolist())
    np.testing.assert_allclose(got, g["losses"], rtol=1e-4)
    np.testing.assert_allclose(torch.stack([x.detach() for x in res["outs"][2]]).cpu().numpy(), g["R"],
                               atol=1e-5)
    ref = dict(zip([str(n) for n in g["grad_names"]], g["grad_norms"]))
    dec_max = max(v for k, v in ref.items() if k.startswith("decoder."))
    enc_max = max(v for k, v in ref.items() if not k.startswith("decoder."))
    checked, seen = 0, set()
    for n, p in r.named_parameters():
        key = "encoder." + n.split(".", 1)[1] if n.startswith(("real_encoder.", "render_encoder.")) else n
        rv = ref[key]
        gv = 0.0 if p.grad is None else float(p.grad.double().norm())
        tol = 1e-3 * dec_max if key.startswith("decoder.") else 2e-2 * enc_max
        assert abs(gv - rv) <= tol + 1e-3 * rv, f"{n}: HIP {gv:.6e} vs reference {rv:.6e}"
        checked += 1
        seen.add(key)
    assert checked == len(ref) == 149 and seen == set(ref)


def test_masked_train_step_reduces_loss_and_is_deterministic():
    """Two TrainStep steps, B=2, 256², 3 iterations, both flags: the loss decreases, and a second
    identical run gives the same losses and parameters bit for bit.

    The step is the configured one, as in test_train_step_deterministic: TrainStep's default
    OneCycleLR, whose warm-up runs step 0 at lr / 25.  A constant 4e-4 from step 0 is not what
    the config trains with, and AdamW's first update at that rate (every weight moves by ≈ lr
    whatever its gradient) overshoots on the synthetic weights with or without masking — measured
    25.09 → 44.86 unmasked and 25.01 → 42.26 masked, against 25.09 → 23.39 and 25.01 → 23.47 with
    the schedule — so it says nothing about the masked path."""
    from scflow_amd.train.step import TrainStep
    batch, points, diam = train_batch(2, 256, seed=8)
    gb = {k: v.cuda() for k, v in batch.items()}
    runs = []
    for _ in range(2):
        r = masked_refiner(3)
        step = TrainStep(r, [p.cuda() for p in points], diam)
        losses = [float(step(gb)["loss"].detach()) for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((losses, [p.detach().clone() for p in r.parameters()]))
    losses = runs[0][0]
    print("losses", losses)
    assert losses[1] < losses[0], losses  # the loss of the second step: after one update
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
