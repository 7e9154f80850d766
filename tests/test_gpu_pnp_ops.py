"""GPU: the batched RANSAC-PnP stages (scflow_pnp_compact / _hypotheses / _score / _refine) and
``ops.pnp_ransac`` end to end against the numpy fp64 restatement (tests/pnp_restatement.py) on
synthetic scenes with a known pose.  Every bound is the contract's:

* compaction and the sampled rows: exact;
* hypotheses on exact flow: every one the GPU calls valid is full-inlier at 3 px under the
  restatement's fp64 scorer; the GPU may call invalid at most the restatement's own invalid ones
  plus 5 % of ``hyps``;
* scores: within the number of points whose fp64 error lies within 1e-2 px of the threshold;
* refinement and the end-to-end pose: within 4·d of the restatement's fp64 run, d = the distance
  between the restatement's fp64 run and its run with fp32 per-point residuals / Jacobians, measured
  on the pose before its rounding to fp32 (one fp32 ulp of t_z ≈ 1 m is 6e-5 mm, more than d); the
  fp32 outputs are exactly that pose rounded.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import pnp_restatement as pr
from tests.pnp_cases import CASE_LARGE, CASE_SQUARE, CASE_WIDE, case

pytest.importorskip("oracle.scflow_oracle")
pytestmark = pytest.mark.gpu

THR = 3.0


def dev(a, dtype=None):
    x = torch.tensor(np.asarray(a))
    return (x if dtype is None else x.to(dtype)).cuda()


@lru_cache(maxsize=None)
def gpu_case(shape):
    """The case's tensors on the GPU plus the GPU's own lift (the 3D points of the contract are
    scflow_lift_points' output), downloaded once for the restatement."""
    from scflow_amd import ops
    c = case(*shape)
    g = {k: dev(c[k]) for k in ("depth", "K", "R_ref", "t_ref", "flow", "flow_c")}
    g["points"] = ops.lift_points(g["depth"], g["K"], g["R_ref"], g["t_ref"])
    g["points_np"] = g["points"].cpu().numpy()
    g["clean"] = dev((c["depth"] > 0) & ~c["moved"], torch.float32)
    return g


@lru_cache(maxsize=None)
def reference_runs(shape, hyps=100, seed=0):
    """Per sample: the restatement end to end on the contaminated flow, all fp64 and with fp32
    per-point arithmetic, and d = their distance in R (Frobenius) and t."""
    c, g = case(*shape), gpu_case(shape)
    out = []
    for b in range(shape[0]):
        corr, _ = pr.correspondences(g["points_np"][b], c["flow_c"][b])
        args = (corr, c["K"][b], c["R_ref"][b], c["t_ref"][b], b, hyps, THR, 10, seed)
        r64, r32 = pr.ransac(*args), pr.ransac(*args, per_point=np.float32)
        out.append(dict(corr=corr, r64=r64, dR=np.linalg.norm(r64["R"] - r32["R"]),
                        dt=np.linalg.norm(r64["t"] - r32["t"])))
    return out


# ------------------------------------------------------------------------------ compaction
@pytest.mark.parametrize("shape", [CASE_SQUARE, CASE_WIDE])
@pytest.mark.parametrize("masked", [False, True])
def test_compaction_is_flatnonzero_order(shape, masked):
    from scflow_amd import ops
    c, g = case(*shape), gpu_case(shape)
    valid = g["clean"] if masked else None
    corr, count = ops.pnp_compact(g["points"], g["flow_c"], valid)
    corr, count = corr.cpu().numpy(), count.cpu().numpy()
    for b in range(shape[0]):
        want, p = pr.correspondences(g["points_np"][b], c["flow_c"][b],
                                     ~c["moved"][b] if masked else None)
        keep = c["depth"][b].reshape(-1) > 0
        if masked:
            keep &= ~c["moved"][b].reshape(-1)
        assert np.array_equal(p, np.flatnonzero(keep))
        assert count[b] == len(want)
        assert np.array_equal(corr[b, :count[b]], want)
    if shape[4] is not None:
        assert count[shape[4]] == 0


# ------------------------------------------------------------------------------ hypotheses
@pytest.mark.parametrize("shape,hyps,seed", [(CASE_SQUARE, 100, 0), (CASE_SQUARE, 37, 11),
                                             (CASE_WIDE, 100, 0), (CASE_WIDE, 37, 11)])
def test_hypotheses_sample_as_the_restatement_and_are_full_inlier(shape, hyps, seed):
    from scflow_amd import ops
    c, g = case(*shape), gpu_case(shape)
    corr, count = ops.pnp_compact(g["points"], g["flow"])
    hyp, pose, hv, samples = ops.pnp_hypotheses(corr, count, g["K"], hyps, seed)
    corr, count, hyp, pose, hv, samples = (x.cpu().numpy() for x in (corr, count, hyp, pose, hv,
                                                                    samples))
    for b in range(shape[0]):
        cb = corr[b, :count[b]]
        ref = pr.hypotheses(cb, c["K"][b], b, hyps, seed)
        assert np.array_equal(samples[b], ref["idx"])
        n_bad = 0
        for h in np.flatnonzero(hv[b]):
            e = pr.reproj_errors(cb, hyp[b, h].reshape(3, 4).astype(np.float64))
            n_bad += int((e < THR).sum() != count[b])
            # hyp = K·[R|t] of hyp_pose
            Rt = pose[b, h].reshape(3, 4).astype(np.float64)
            np.testing.assert_allclose(c["K"][b].astype(np.float64) @ Rt,
                                       hyp[b, h].reshape(3, 4), rtol=1e-5, atol=1e-2)
        gpu_invalid, ref_invalid = int((hv[b] == 0).sum()), int((~ref["valid"]).sum())
        print(f"{shape} hyps {hyps} sample {b}: count {count[b]}, invalid GPU {gpu_invalid} / "
              f"restatement {ref_invalid}, valid but not full-inlier {n_bad}")
        assert n_bad == 0
        assert gpu_invalid <= ref_invalid + int(0.05 * hyps)
        if count[b] == 0:
            assert gpu_invalid == hyps


def test_hypotheses_beyond_the_largest_count_are_unsupported():
    from scflow_amd import ops
    from scflow_amd._lib import ScflowError
    g = gpu_case(CASE_SQUARE)
    corr, count = ops.pnp_compact(g["points"], g["flow"])
    with pytest.raises(ScflowError, match="unsupported"):
        ops.pnp_hypotheses(corr, count, g["K"], ops.PNP_MAX_HYPS + 1)
    ops.pnp_hypotheses(corr, count, g["K"], ops.PNP_MAX_HYPS)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ scoring
@pytest.mark.parametrize("shape,hyps", [(CASE_SQUARE, 100), (CASE_WIDE, 37),
                                        (CASE_LARGE, 255)])  # + 1 = the largest supported
def test_scores_match_the_fp64_count_within_the_threshold_band(shape, hyps):
    from scflow_amd import ops
    c, g = case(*shape), gpu_case(shape)
    corr, count = ops.pnp_compact(g["points"], g["flow_c"])
    corr_np, count_np = corr.cpu().numpy(), count.cpu().numpy()
    B = shape[0]
    P = np.zeros((B, hyps + 1, 12), np.float32)
    valid = np.zeros((B, hyps + 1), np.int32)
    for b in range(B):
        ref = pr.hypotheses(corr_np[b, :count_np[b]], c["K"][b], b, hyps, 0)
        P[b, :hyps] = ref["P"].reshape(hyps, 12)
        valid[b, :hyps] = ref["valid"]
        # one more: a valid pose with the translation negated puts every point behind the camera
        w = int(np.argmax(ref["valid"]))
        Rt = np.concatenate([ref["R"][w], -ref["t"][w][:, None] if ref["valid"][w]
                             else -np.array([[0.0], [0.0], [1000.0]])], 1)
        P[b, hyps] = (c["K"][b].astype(np.float64) @ Rt).reshape(12)
        valid[b, hyps] = 1
    score = ops.pnp_score(corr, count, dev(P), dev(valid), THR).cpu().numpy()
    for b in range(B):
        cb = corr_np[b, :count_np[b]]
        want, band = pr.score(cb, P[b].astype(np.float64).reshape(-1, 3, 4), valid[b] != 0, THR)
        diff = np.abs(score[b] - want)
        print(f"{shape} sample {b}: count {count_np[b]}, points within 1e-2 px of the threshold "
              f"{band.sum()} (max per hypothesis {band.max()}), score differences {diff.sum()}")
        assert band.max() <= 0.01 * max(count_np[b], 1)  # the seeds' precondition
        assert (diff <= band).all()
        assert score[b, hyps] == 0 and want[hyps] == 0
        assert (score[b][valid[b] == 0] == 0).all()
        assert score[b].max() <= count_np[b]


# ------------------------------------------------------------------------------ refinement
@pytest.mark.parametrize("shape", [CASE_SQUARE, CASE_WIDE])
def test_refinement_within_four_d_of_the_fp64_run(shape):
    from scflow_amd import ops
    c, g = case(*shape), gpu_case(shape)
    corr, count = ops.pnp_compact(g["points"], g["flow_c"])
    B = shape[0]
    runs = reference_runs(shape, 100)
    P = np.zeros((B, 1, 12), np.float32)
    Rt = np.zeros((B, 1, 12), np.float32)
    valid, score = np.zeros((B, 1), np.int32), np.zeros((B, 1), np.int32)
    want = []
    for b in range(B):
        r64, cb = runs[b]["r64"], runs[b]["corr"]
        if not r64["ok"]:
            want.append(None)
            continue
        w, K = r64["winner"], c["K"][b].astype(np.float64)
        # the start the kernel sees: the restatement's winner rounded to fp32
        R0, t0 = r64["hyp"]["R"][w].astype(np.float32), r64["hyp"]["t"][w].astype(np.float32)
        Rt[b, 0] = np.concatenate([R0, t0[:, None]], 1).reshape(12)
        P[b, 0] = r64["hyp"]["P"][w].reshape(12)
        e = pr.reproj_errors(cb, P[b, 0].astype(np.float64).reshape(3, 4))
        assert not (np.abs(e - THR) <= 1e-2).any()  # the inlier set is the same in fp32
        inl = e < THR
        valid[b, 0], score[b, 0] = 1, inl.sum()
        a = (cb, inl, R0.astype(np.float64), t0.astype(np.float64), K, 10)
        f64, f32 = pr.refine(*a), pr.refine(*a, per_point=np.float32)
        want.append((f64, np.linalg.norm(f64[0] - f32[0]), np.linalg.norm(f64[1] - f32[1])))
    pose64 = torch.zeros(B, 12, device="cuda", dtype=torch.float64)
    R, t, ok, inl = ops.pnp_refine(corr, count, dev(P), dev(Rt), dev(valid), dev(score), g["K"],
                                   g["R_ref"], g["t_ref"], THR, 10, pose64)
    R, t, ok, inl, p64 = (x.cpu().numpy() for x in (R, t, ok, inl, pose64))
    for b in range(B):
        if want[b] is None:
            assert ok[b] == 0 and inl[b] == 0
            assert R[b].tobytes() == c["R_ref"][b].tobytes()
            assert t[b].tobytes() == c["t_ref"][b].tobytes()
            continue
        (R64, t64), dR, dt = want[b]
        gR = np.linalg.norm(p64[b, :9].reshape(3, 3) - R64)
        gt = np.linalg.norm(p64[b, 9:] - t64)
        print(f"{shape} sample {b}: d = {dR:.2e} (R), {dt:.2e} mm (t); GPU vs fp64 {gR:.2e}, "
              f"{gt:.2e} mm")
        assert ok[b] == 1 and inl[b] == score[b, 0]
        assert gR <= 4 * dR and gt <= 4 * dt
        assert np.array_equal(R[b], p64[b, :9].reshape(3, 3).astype(np.float32))
        assert np.array_equal(t[b], p64[b, 9:].astype(np.float32))


# ------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("shape,hyps", [(CASE_SQUARE, 100), (CASE_WIDE, 37), (CASE_LARGE, 100)])
def test_pnp_ransac_on_contaminated_flow(shape, hyps):
    from scflow_amd import ops
    c, g = case(*shape), gpu_case(shape)
    B = shape[0]
    runs = reference_runs(shape, hyps)
    pose64 = torch.zeros(B, 12, device="cuda", dtype=torch.float64)
    R, t, ok, inl = ops.pnp_ransac(g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"],
                                   hyps=hyps, thr=THR, pose64=pose64)
    assert ok.dtype == torch.bool and inl.dtype == torch.int32
    assert tuple(R.shape) == (B, 3, 3) and tuple(t.shape) == (B, 3)
    R, t, ok, inl, p64 = (x.cpu().numpy() for x in (R, t, ok, inl, pose64))
    for b in range(B):
        if b == shape[4]:  # the empty sample: the reference pose, bit for bit
            assert not ok[b] and inl[b] == 0
            assert R[b].tobytes() == c["R_ref"][b].tobytes()
            assert t[b].tobytes() == c["t_ref"][b].tobytes()
            continue
        r64 = runs[b]["r64"]
        clean = int(((c["depth"][b] > 0) & ~c["moved"][b]).sum())
        gR = np.linalg.norm(p64[b, :9].reshape(3, 3) - r64["R"])
        gt = np.linalg.norm(p64[b, 9:] - r64["t"])
        print(f"{shape} sample {b}: inliers {inl[b]} of {clean} clean; d = {runs[b]['dR']:.2e} (R), "
              f"{runs[b]['dt']:.2e} mm (t); GPU vs restatement {gR:.2e}, {gt:.2e} mm")
        assert ok[b] and r64["ok"]
        assert inl[b] == clean == r64["inliers"]
        assert gR <= 4 * runs[b]["dR"] and gt <= 4 * runs[b]["dt"]
        assert np.array_equal(R[b], p64[b, :9].reshape(3, 3).astype(np.float32))
        assert np.array_equal(t[b], p64[b, 9:].astype(np.float32))


def test_validity_mask_removes_the_contaminated_pixels():
    from scflow_amd import ops
    g = gpu_case(CASE_SQUARE)
    _, count = ops.pnp_compact(g["points"], g["flow_c"], g["clean"])
    for valid in (g["clean"], g["clean"] != 0):  # float and bool masks
        R, t, ok, inl = ops.pnp_ransac(g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"],
                                       valid=valid)
        assert ok.tolist() == [True, True, False]
        assert torch.equal(inl, torch.where(ok, count, torch.zeros_like(count)))


def test_repeated_calls_and_a_graph_replay_are_bit_identical():
    """Captured on one stream into a graph and replayed: equal to the eager call bit for bit, so
    nothing between the stages waits for the host."""
    from scflow_amd import ops
    g = gpu_case(CASE_SQUARE)
    args = (g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"])
    eager = ops.pnp_ransac(*args)
    again = ops.pnp_ransac(*args)
    for a, b in zip(eager, again):
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.pnp_ransac(*args)  # allocator warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = ops.pnp_ransac(*args)
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    assert eager[2].tolist() == [True, True, False]


def test_opcheck_pnp_ransac():
    from scflow_amd import library  # noqa: F401  (registers the op)
    g = gpu_case(CASE_SQUARE)
    args = (g["flow_c"], g["depth"], g["R_ref"], g["t_ref"], g["K"], None, 37, THR, 10, 0)
    torch.library.opcheck(torch.ops.scflow.pnp_ransac.default, args)
    torch.library.opcheck(torch.ops.scflow.pnp_ransac.default,
                          args[:5] + (g["clean"], 100, THR, 10, 5))
    R, t, ok, inl = torch.ops.scflow.pnp_ransac(*args)
    want = library.ops.pnp_ransac(*args[:5], hyps=37)
    for a, b in zip((R, t, ok, inl), want):
        assert torch.equal(a, b)
