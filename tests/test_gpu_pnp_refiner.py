"""GPU: the RAFT refiners' pose half — ``solve_pose`` (the reference's dict layout on the batched
RANSAC-PnP) and ``get_pose`` (``get_flow`` + PnP on the last flow)."""
import numpy as np
import pytest
import torch

from tests.pnp_cases import CASE_SQUARE, case
from tests.test_gpu_pnp_ops import dev, gpu_case
from tests.test_gpu_raft_refiner import build_refiner, model_cfg

pytest.importorskip("oracle.scflow_oracle")
pytestmark = pytest.mark.gpu


def _refiner(**test_cfg):
    from scflow_amd import MODELS
    cfg = model_cfg("RAFTRefinerFlowMask", False)
    cfg["test_cfg"] = dict(iters=2, **test_cfg)
    return MODELS.build(cfg)


def test_solve_pose_returns_the_reference_layout_and_drops_failed_samples():
    from scflow_amd import ops
    g = gpu_case(CASE_SQUARE)
    labels = torch.tensor([4, 9, 17]).cuda()
    r = _refiner(solve_pose_param=dict(reprojectionerror=3.0, iterationscount=37))
    out = r.solve_pose(g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"], labels, [2, 1])
    R, t, ok, _ = ops.pnp_ransac(g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"], hyps=37)
    assert ok.tolist() == [True, True, False]  # sample 2 has no depth
    assert sorted(out) == ["labels", "rotations", "scores", "translations"]
    for v in out.values():
        assert isinstance(v, list) and len(v) == 2
    assert torch.equal(out["rotations"][0], R[:2]) and tuple(out["rotations"][1].shape) == (0, 3, 3)
    assert torch.equal(out["translations"][0], t[:2])
    assert tuple(out["translations"][1].shape) == (0, 3)
    assert out["labels"][0].tolist() == [4, 9] and out["labels"][1].tolist() == []
    assert out["scores"][0].tolist() == [1.0, 1.0] and out["scores"][0].dtype == torch.float32
    assert out["scores"][1].numel() == 0
    # the reference's defaults: 100 hypotheses at 3 px
    out = _refiner().solve_pose(g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"], labels,
                                torch.tensor([1, 2]))
    R, t, _, _ = ops.pnp_ransac(g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"])
    assert torch.equal(out["rotations"][0], R[:1]) and torch.equal(out["rotations"][1], R[1:2])
    assert torch.equal(out["translations"][1], t[1:2]) and out["labels"][1].tolist() == [9]


def test_solve_pose_excludes_pixels_below_the_occlusion_threshold():
    from scflow_amd import ops
    c, g = case(*CASE_SQUARE), gpu_case(CASE_SQUARE)
    labels = torch.zeros(3, dtype=torch.long).cuda()
    # confident where the flow is clean, 0.45 (below occ_thresh = 0.5, above 0.4) where it was moved
    occ = dev(np.where(c["moved"], 0.45, 0.9).astype(np.float32))[:, None]
    clean = [int(((c["depth"][b] > 0) & ~c["moved"][b]).sum()) for b in range(3)]
    total = [int((c["depth"][b] > 0).sum()) for b in range(3)]
    r = _refiner()
    R, t, ok, inl = r._pnp(g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"], occ)
    assert inl.tolist() == [clean[0], clean[1], 0]
    want = ops.pnp_ransac(g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"],
                          valid=occ[:, 0] > 0.5)
    assert torch.equal(R, want[0]) and torch.equal(t, want[1])
    out = r.solve_pose(g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"], labels, [3], occ)
    assert torch.equal(out["rotations"][0], R[:2]) and torch.equal(out["translations"][0], t[:2])
    # the exact flow under a lower threshold: the moved pixels count again
    _, _, _, inl = _refiner(occ_thresh=0.4)._pnp(g["flow"], g["depth"], g["R_ref"], g["t_ref"],
                                                 g["K"], occ)
    assert inl.tolist() == [total[0], total[1], 0]
    # sample_points thins the set to at most num pixels
    _, _, ok, inl = _refiner(sample_points=dict(mode="topk", num=300))._pnp(
        g["flow"], g["depth"], g["R_ref"], g["t_ref"], g["K"], occ)
    assert ok.tolist() == [True, True, False] and inl.tolist() == [300, 300, 0]


def test_get_pose_runs_the_flow_network_then_pnp():
    """B=2 at 256², the smallest image the flow network's kernels take: at 64² the encoder's last
    stage is 8 × 8, below scflow_enc_conv's smallest tile, and at 128² the decoder's GRU has no
    conv kernel for 16-wide feature maps (both refuse loudly, SCFLOW_EUNSUPPORTED / ScflowError,
    seen on the MI355X)."""
    from tests.helpers import refine_inputs
    inp = refine_inputs(2, 256, seed=13, device="cuda")
    r, _ = build_refiner("RAFTRefinerFlowMask", False)
    R, t, ok, inl = r.get_pose(inp["render_images"], inp["real_images"], inp["depth"],
                               inp["ref_rotation"], inp["ref_translation"], inp["internel_k"])
    torch.cuda.synchronize()
    assert tuple(R.shape) == (2, 3, 3) and tuple(t.shape) == (2, 3)
    assert tuple(ok.shape) == (2,) and ok.dtype == torch.bool
    assert tuple(inl.shape) == (2,) and inl.dtype == torch.int32
    assert torch.isfinite(R).all() and torch.isfinite(t).all()
    assert r.decoder.iters == 4  # test_iter_num (12) applies to the call only
    for b in range(2):
        if not ok[b]:
            assert torch.equal(R[b], inp["ref_rotation"][b]) and inl[b] == 0
            assert torch.equal(t[b], inp["ref_translation"][b])
        else:
            assert 4 <= int(inl[b]) <= int((inp["depth"][b] > 0).sum())
            np.testing.assert_allclose((R[b] @ R[b].T).cpu().numpy(), np.eye(3), atol=1e-5)
