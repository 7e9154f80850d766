"""CPU: the RANSAC-PnP contract's restatement (tests/pnp_restatement.py) recovers a known pose,
its sampling hash has the stated fixed vectors, the C ABI / ctypes / library layers agree on the new
exports, the workspace query answers without a GPU, and the refiner's ``solve_pose`` plumbing
(refusals, ``sample_points``) behaves as documented."""
import os
import re

import numpy as np
import pytest
import torch

from tests import pnp_restatement as pr
from tests.pnp_cases import CASE_SQUARE, CASE_WIDE, case

pytest.importorskip("oracle.scflow_oracle")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNP_EXPORTS = ("scflow_pnp_workspace", "scflow_pnp_compact", "scflow_pnp_hypotheses",
               "scflow_pnp_score", "scflow_pnp_refine")

# Pose error allowed against the ground truth on noise-free inputs.  The inputs are exact up to one
# fp32 rounding: u, v below 128 px carry ≤ 4e-6 px, the lifted points (≤ 150 mm, ulp 1.5e-5 mm,
# projected with f/z ≈ 1 px/mm) ≈ 1e-5 px.  A pixel error e on an object of radius ≈ 25 px turns
# the pose by ≤ e/25 ≈ 4e-7 rad and moves t_z ≈ 1000 mm by ≤ t_z·e/25 ≈ 4e-4 mm even without any
# averaging over the ≈ 1000 points; the bounds leave a factor 25 over that.
R_TOL, T_TOL = 1e-5, 1e-2


def test_lowbias32_fixed_vectors():
    want = {0: 0x0, 1: 0x688990C0, 2: 0xD1132181, 0xFFFFFFFF: 0x6768824A, 0xDEADBEEF: 0xE628C683,
            12345: 0x912EFCF7}
    for x, y in want.items():
        assert int(pr.lowbias32(x)) == y, hex(x)
    got = pr.lowbias32(np.array(list(want), np.uint64))
    assert [int(v) for v in got] == list(want.values())


def test_sample_indices_fixed_vectors():
    # (lowbias32(((b·hyps + h)·4 + k) ^ seed) · count) >> 32 at b = 1, hyps = 3, count = 1000, seed = 7
    assert pr.sample_indices(1, 3, 1000, 7).tolist() == [[16, 720, 260, 915], [167, 549, 286, 140],
                                                         [104, 37, 299, 131]]
    idx = pr.sample_indices(0, 100, 17, 0)
    assert idx.shape == (100, 4) and idx.min() >= 0 and idx.max() < 17
    assert not pr.sample_indices(5, 8, 0, 3).any()  # an empty sample draws row 0 four times


@pytest.mark.parametrize("shape", [CASE_SQUARE, CASE_WIDE])
@pytest.mark.parametrize("contaminated", [False, True])
def test_restatement_recovers_the_ground_truth_pose(shape, contaminated):
    c = case(*shape)
    for b in range(shape[0]):
        corr, _ = pr.correspondences(c["points"][b], c["flow_c" if contaminated else "flow"][b])
        res = pr.ransac(corr, c["K"][b], c["R_ref"][b], c["t_ref"][b], b)
        if b == shape[4]:
            assert len(corr) == 0 and not res["ok"] and res["inliers"] == 0
            assert res["R"] is not None and np.array_equal(res["R"], c["R_ref"][b])
            continue
        clean = int(((c["depth"][b] > 0) & ~(c["moved"][b] & contaminated)).sum())
        dR = np.linalg.norm(res["R"] - c["R_gt"][b].astype(np.float64))
        dt = np.linalg.norm(res["t"] - c["t_gt"][b].astype(np.float64))
        print(f"{shape} sample {b}: count {len(corr)}, inliers {res['inliers']}, |dR| {dR:.2e}, "
              f"|dt| {dt:.2e} mm")
        assert res["ok"] and res["inliers"] == clean
        assert dR <= R_TOL and dt <= T_TOL


def test_restatement_hypotheses_are_full_inlier_on_exact_flow():
    c = case(*CASE_SQUARE)
    for b in range(2):
        corr, _ = pr.correspondences(c["points"][b], c["flow"][b])
        hyp = pr.hypotheses(corr, c["K"][b], b, 100, 0)
        sc, _ = pr.score(corr, hyp["P"], hyp["valid"])
        assert (~hyp["valid"]).sum() <= 5
        assert (sc[hyp["valid"]] == len(corr)).all()
        assert (sc[~hyp["valid"]] == 0).all()


def test_header_signatures_and_library_agree_on_the_pnp_exports():
    from scflow_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scflow_hip.h")).read(),
                 flags=re.S)
    declared = set(re.findall(r"\b(scflow_pnp_[a-z0-9_]+)\s*\(", src))
    assert declared == set(PNP_EXPORTS)
    assert re.search(r"#define\s+SCFLOW_ABI_VERSION\s+4\b", src)
    m = re.search(r"#define\s+SCFLOW_PNP_MAX_HYPS\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.PNP_MAX_HYPS >= 256
    lib = _lib.load()
    assert lib.scflow_abi_version() == 4 == _lib.ABI_VERSION
    for name in PNP_EXPORTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # argument counts of the declarations and of the ctypes signatures
    for name in PNP_EXPORTS:
        args = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_workspace_query_needs_no_gpu():
    import ctypes
    from scflow_amd import _lib, ops
    lib = _lib.load()
    nb = ctypes.c_longlong(-1)
    assert lib.scflow_pnp_workspace(16, 256, 256, 100, ctypes.byref(nb)) == 0
    assert nb.value == 16 * 64 * 4  # one int per 1024-pixel chunk
    assert ops.pnp_workspace_bytes(3, 64, 64, 256) == 48
    assert ops.pnp_workspace_bytes(1, 5, 7, 1) == 16  # rounded up to 16 bytes
    assert lib.scflow_pnp_workspace(1, 64, 64, 257, ctypes.byref(nb)) == -2  # beyond the largest hyps
    assert lib.scflow_pnp_workspace(1, 64, 64, 100, None) == -1
    assert lib.scflow_pnp_workspace(0, 64, 64, 100, ctypes.byref(nb)) == -1
    # argument errors return codes before anything is launched
    assert lib.scflow_pnp_compact(None, None, None, None, None, None, 0, 1, 8, 8, None) == -1
    assert lib.scflow_pnp_hypotheses(None, None, None, None, None, None, None, 1, 64, 100, 0, None) == -1
    assert lib.scflow_pnp_score(None, None, None, None, None, 1, 64, 100, 3.0, None) == -1
    assert lib.scflow_pnp_refine(*([None] * 14), 1, 64, 100, 3.0, 10, None) == -1
    with pytest.raises(_lib.ScflowError):
        ops.pnp_workspace_bytes(1, 64, 64, 1000)


def _refiner(**test_cfg):
    from scflow_amd import MODELS
    from tests.test_gpu_raft_refiner import model_cfg
    cfg = model_cfg("RAFTRefinerFlowMask", False)
    cfg["test_cfg"] = dict(iters=2, **test_cfg)
    return MODELS.build(cfg)


@pytest.mark.parametrize("test_cfg", [dict(solve_pose_mode="progressive-x"),
                                      dict(solve_pose_space="origin"),
                                      dict(solve_pose_mode="epnp")])
def test_solve_pose_refuses_what_is_not_built(test_cfg):
    from scflow_amd._lib import ScflowError
    r = _refiner(**test_cfg)
    z = torch.zeros(1, 2, 8, 8)
    with pytest.raises(ScflowError):
        r.solve_pose(z, z[:, 0], torch.eye(3)[None], torch.zeros(1, 3), torch.eye(3)[None],
                     torch.zeros(1, dtype=torch.long), [1])


def test_solve_pose_refuses_cpu_tensors():
    from scflow_amd._lib import ScflowError
    z = torch.zeros(1, 2, 8, 8)
    with pytest.raises(ScflowError):
        _refiner().solve_pose(z, z[:, 0], torch.eye(3)[None], torch.zeros(1, 3), torch.eye(3)[None],
                              torch.zeros(1, dtype=torch.long), [1])


def test_sample_points_thins_the_mask_to_num():
    g = torch.Generator().manual_seed(3)
    depth = (torch.rand(3, 16, 20, generator=g) > 0.4).float()
    depth[2, :, :] = 0
    depth[2, 0, :5] = 1.0  # fewer candidates than num: all of them stay
    occ = torch.rand(3, 1, 16, 20, generator=g)
    # no sample_points: the occlusion threshold alone (None without an occlusion)
    r = _refiner(occ_thresh=0.25)
    assert r._pnp_valid(None, depth) is None
    assert torch.equal(r._pnp_valid(occ, depth), occ[:, 0] > 0.25)
    for mode in ("random", "topk"):
        r = _refiner(sample_points=dict(mode=mode, num=40))
        keep = r._pnp_valid(occ, depth)
        cand = (depth > 0) & (occ[:, 0] > 0.5)
        assert keep.dtype == torch.bool and keep.shape == depth.shape
        assert not (keep & ~cand).any()
        assert keep.flatten(1).sum(1).tolist() == [40, 40, int(cand[2].sum())]
        if mode == "topk":  # the 40 most confident candidates
            for b in range(2):
                conf = occ[b, 0][cand[b]]
                assert occ[b, 0][keep[b]].min() >= conf.sort(descending=True).values[39]
    # random needs no occlusion; topk does
    keep = _refiner(sample_points=dict(mode="random", num=7))._pnp_valid(None, depth)
    assert keep.flatten(1).sum(1).tolist() == [7, 7, 5]
    from scflow_amd._lib import ScflowError
    with pytest.raises(ScflowError):
        _refiner(sample_points=dict(mode="topk", num=7))._pnp_valid(None, depth)
