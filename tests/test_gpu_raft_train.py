"""GPU: training of the RAFT baseline on the HIP autograd Functions (B = 2, 256², 3 iterations).

* ``raft_refiner_train_forward`` + ``backward`` against the fixture written from the REFERENCE's
  own modules in train mode (tests/golden/make_golden_raft_train.py), three variants, with the
  tolerances of tests/test_gpu_train.py's reference-fixture test (tests/raft_train_restatement.py
  ``check_against_fixture``);
* ``raft_decoder_train``'s ×8 flows and occlusions against the inference ``_forward`` of the same
  decoder on the same features (the path that already has reference parity);
* two ``TrainStep`` steps lower the loss and are bitwise reproducible; ``loss`` returns the
  reference's ``log_vars``; graph mode is refused.
"""
import pytest
import torch

from tests import raft_restatement as rr
from tests import raft_train_restatement as rt
from tests.test_train_host import train_batch

pytestmark = pytest.mark.gpu
orc = pytest.importorskip("oracle.scflow_oracle")


def _fixture_batch():
    B, S, _, seed, labels, _ = rt.fixture_meta()
    batch, _, _ = train_batch(B, S, seed=seed, labels=labels)
    return {k: v.cuda() for k, v in batch.items()}


@pytest.mark.parametrize("tag", ["mask", "plain", "bilinear"])
def test_train_forward_backward_matches_reference_fixture(tag):
    from scflow_amd.train.model import raft_refiner_train_forward
    r = rt.build_train_refiner(tag).cuda()
    res = raft_refiner_train_forward(r, _fixture_batch())
    res["loss"].backward()
    torch.cuda.synchronize()
    rt.check_against_fixture(tag, res, r)


@pytest.mark.parametrize("kind,over", [("RAFTDecoderMask", {}), ("RAFTDecoder", {}),
                                       ("RAFTDecoderMask", dict(convex_unsample_flow=False))],
                         ids=["mask", "plain", "bilinear"])
def test_train_forward_equals_inference_forward(kind, over):
    """Mean EPE ≤ 1e-3 px on every iteration's ×8 flow, occlusion max difference ≤ 1e-5."""
    from scflow_amd.train.model import raft_decoder_train
    iters = 3
    dec = rr.build_raft_decoder(kind, iters=iters, **over).cuda()
    inp = {k: v.cuda() for k, v in rr.raft_inputs(2, 256, seed=11).items()}
    with torch.no_grad():
        out = dec._forward(inp["feat1"], inp["feat2"], inp["flow"], inp["h_feat"], inp["cxt_feat"])
    inf_flow, inf_occ = out if kind == "RAFTDecoderMask" else (out, [])
    cl = lambda a: a.permute(0, 2, 3, 1).contiguous()  # noqa: E731
    dec.train()
    upflows, upoccs, lr_flows = raft_decoder_train(dec, cl(inp["feat1"]), cl(inp["feat2"]),
                                                   cl(inp["h_feat"]), cl(inp["cxt_feat"]), iters)
    torch.cuda.synchronize()
    assert len(upflows) == len(lr_flows) == iters and len(upoccs) == len(inf_occ)
    assert upflows[-1].requires_grad
    for i in range(iters):
        epe = rr.mean_epe(inf_flow[i].cpu(), upflows[i].detach().cpu())
        print(f"{kind} {over}: iteration {i}: train vs inference upflow mean EPE {epe:.3e} px")
        assert epe <= rr.EPE_TOL, i
    for i, (a, b) in enumerate(zip(inf_occ, upoccs)):
        d = float((a - b.detach()).abs().max())
        print(f"{kind} {over}: iteration {i}: occlusion max difference {d:.3e}")
        assert d <= 1e-5, i


def _two_steps():
    from scflow_amd.train.step import TrainStep
    r = rt.build_train_refiner("mask").cuda()
    batch, _, _ = train_batch(2, 256, seed=8)
    gb = {k: v.cuda() for k, v in batch.items()}
    step = TrainStep(r, None, None, max_norm=1.0)  # the default OneCycle warm-up
    losses = [float(step(gb)["loss"]) for _ in range(2)]
    torch.cuda.synchronize()
    return losses, [p.detach().clone() for p in r.parameters()]


def test_two_train_steps_lower_the_loss_and_are_bitwise_reproducible():
    """Reference modules on the CPU, same schedule: 177.19 → 164.44 (→ 159.09)."""
    losses, params = _two_steps()
    print("RAFTRefinerFlowMask, two steps:", losses)
    assert losses[1] < losses[0], losses
    assert all(bool(torch.isfinite(p).all()) for p in params)
    losses2, params2 = _two_steps()
    assert losses2 == losses
    assert all(torch.equal(a, b) for a, b in zip(params, params2))


def test_loss_returns_the_reference_log_vars_and_graph_mode_is_refused():
    from scflow_amd.train.step import TrainStep
    _, _, iters, _, _, _ = rt.fixture_meta()
    r = rt.build_train_refiner("mask").cuda()
    loss, imgs, log_vars = r.loss(_fixture_batch())
    assert imgs is None and loss.requires_grad
    want = [k for i in range(iters) for k in (f"seq_{i}_flow_loss", f"seq_{i}_occ_loss")] + \
        ["loss_occ", "loss_flow", "loss"]
    assert list(log_vars) == want
    assert all(isinstance(v, float) for v in log_vars.values())
    g = rt.raft_train_golden()
    assert log_vars["loss"] == pytest.approx(float(g["mask_losses"][0]), rel=1e-4)
    assert log_vars["loss"] == pytest.approx(float(loss.detach()), rel=1e-6)
    with pytest.raises(NotImplementedError, match="graph"):
        TrainStep(r, None, None, graph=True)
    # the plain refiner has no occlusion terms
    _, _, lv = rt.build_train_refiner("plain").cuda().loss(_fixture_batch())
    assert list(lv) == [f"seq_{i}_flow_loss" for i in range(iters)] + ["loss_flow", "loss"]
