"""GPU: ``scflow_flow_gt`` / ``scflow_flow_epe`` (scflow_amd/csrc/flow_eval.hip) through
``scflow_amd.flow_eval`` against the float64 restatement (``tests/flow_eval_restatement.py``) on
its three shapes: N = 4 at 64² (the golden batch), N = 3 at 20 × 36 (non-square, H·W no multiple
of 256, one sample without depth) and N = 1 at 8².

Gates.  Validity decisions are identical outside the near-decision pixels of the
restatement, which are at most 1 % of the pixels; a count differs by at most the excluded pixels of
its sample; the filtered flow has the unfiltered flow's bits where both say valid.  Error means and
the error map: four times the deviation of the reference's own float32 CPU run from its float64 run
on the same inputs (``golden_flow_eval.npz`` ``dev_<case>``: one factor 2 for another summation
order, one for headroom).  The occlusion mean: 2^-25, the rounding of one float32 subtraction of
numbers in [0, 1] (the fp64 accumulation adds nothing visible).

Measured on the MI355X (profiles/flow_eval/gputest.log): see DESIGN.md §27."""
import os

import numpy as np
import pytest
import torch

from tests import flow_eval_restatement as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_flow_eval.npz")
INV = 400.0
NEAR_MAX = 0.01
OCC_TOL = 2.0 ** -25


def note(line):
    """A measured figure, printed before its assertion (``pytest -s`` shows it)."""
    print(line)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


_CACHE = {}


def scene(name):
    """(CPU batch, its tensors on the GPU, the kernel's unfiltered flow, that flow on the CPU)."""
    if name not in _CACHE:
        from scflow_amd import flow_eval
        b = fr.scene_case(name)
        d = {k: v.cuda() for k, v in b.items()}
        flow, _ = flow_eval.gt_flow(d["depth"], d["internel_k"], d["ref_rotation"], d["ref_translation"],
                                    d["gt_rotation"], d["gt_translation"], INV)
        _CACHE[name] = (b, d, flow, flow.cpu())
    return _CACHE[name]


def poses(d):
    return (d["depth"], d["internel_k"], d["ref_rotation"], d["ref_translation"], d["gt_rotation"],
            d["gt_translation"])


def invalid(flow):
    return (flow[:, 0] == INV) & (flow[:, 1] == INV)


def check_filtered(tag, src, got, bad, near):
    """The gates of a filtered flow ``got`` (GPU) of ``src`` against the restatement's (bad, near)."""
    src, got = src.cpu(), got.cpu()
    share = float(near.double().mean())
    differ = int(((invalid(got) != (bad | invalid(src))) & ~near).sum())
    keep = ~bad & ~near & ~invalid(got)
    same_bits = bool(torch.equal(got.permute(0, 2, 3, 1)[keep], src.permute(0, 2, 3, 1)[keep]))
    rewritten = bad & ~near
    at_invalid = bool((got.permute(0, 2, 3, 1)[rewritten] == INV).all())
    note(f"{tag}: near-decision share {share:.4f}, decisions differing outside it {differ}, invalid "
         f"{int(bad.sum())} of {bad.numel()}, valid pixels keep their bits {same_bits}")
    assert share <= NEAR_MAX
    assert differ == 0
    assert same_bits and at_invalid


# ------------------------------------------------------------------------------------ the flow
@pytest.mark.parametrize("name", fr.CASES)
def test_unfiltered_flow_is_lift_points_plus_pose_flow(name):
    from scflow_amd import flow_eval, ops
    b, d, flow, flow_cpu = scene(name)
    pts = ops.lift_points(d["depth"], d["internel_k"], d["ref_rotation"], d["ref_translation"])
    two = ops.pose_flow(d["gt_rotation"], d["gt_translation"], d["internel_k"], pts, INV)
    assert torch.equal(flow, two)
    both = flow_eval.gt_flow(*poses(d), INV)
    assert torch.equal(both[0], flow) and torch.equal(both[1], flow)  # no filter: a copy
    rest = fr.scene_gt_flow(b)
    assert torch.equal(invalid(flow_cpu), b["depth"] <= 0)
    v = b["depth"] > 0
    dev = float((flow_cpu.double() - rest).abs().amax(1)[v].max()) if v.any() else 0.0
    note(f"gt_flow {name}: largest |fp32 kernel − fp64 restatement| over valid pixels {dev:.3e} px")
    assert dev < 1e-2  # a plausibility bound only: the bits are pinned by the equality above


FILTERS = ("mask", "depth_or", "depth_reference", "face", "all_or", "all_reference")


def run_filter(which, b, d, src, source_b):
    """(GPU filtered flow, restatement bad, near) of one filter configuration on the flow ``src``."""
    from scflow_amd import ops
    src_cpu = src.cpu()
    kw, bad = {}, torch.zeros_like(src_cpu[:, 0], dtype=torch.bool)
    near = torch.zeros_like(bad)
    combine = "reference" if which.endswith("reference") else "or"
    if which in ("mask", "all_or", "all_reference"):
        kw["gt_mask"] = d["gt_masks"]
        k, n = fr.mask_filter(src_cpu, b["gt_masks"])
        bad, near = bad | k, near | n
    if which.startswith("depth") or which.startswith("all"):
        kw.update(depth1=d["gt_depth"], depth_combine=combine)
        k, n = fr.depth_filter(src_cpu, b["gt_depth"], b["depth"], combine=combine)
        bad, near = bad | k, near | n
    if which in ("face", "all_or", "all_reference"):
        kw.update(face_index1=d["face_index"], face_index2=d["gt_face_index"])
        k, n = fr.face_filter(src_cpu, b["face_index"], b["gt_face_index"])
        bad, near = bad | k, near | n
    if source_b:
        need_depth = "depth1" in kw
        got = ops.flow_gt(depth=d["depth"] if need_depth else None, flow_in=src, invalid_num=INV,
                          want_flow=False, **kw)[1]
    else:
        got = ops.flow_gt(*poses(d), invalid_num=INV, **kw)[1]
    return got, bad, near


@pytest.mark.parametrize("which", FILTERS)
@pytest.mark.parametrize("name", fr.CASES)
def test_filters_against_the_restatement(name, which):
    b, d, flow, _ = scene(name)
    got_a, bad, near = run_filter(which, b, d, flow, source_b=False)
    check_filtered(f"{name} {which} (poses)", flow, got_a, bad, near)
    got_b, _, _ = run_filter(which, b, d, flow, source_b=True)
    assert torch.equal(got_a, got_b)  # source (b) on the same flow
    # already-invalid pixels above invalid_num, on the object too: the reference's & is observable
    marked = fr.mark_invalid(flow)
    got_m, bad_m, near_m = run_filter(which, b, d, marked, source_b=True)
    check_filtered(f"{name} {which} (marked flow)", marked, got_m, bad_m, near_m)
    if which == "depth_reference" and name != "tiny":
        assert int((got_m != marked).any(1).sum()) > 0
        assert torch.equal(got_a, flow)  # a no-op on a freshly built GT flow


def test_public_filter_functions_and_mask_dtypes():
    from scflow_amd import flow_eval
    b, d, flow, _ = scene("rect")
    keep = flow.clone()
    want = run_filter("mask", b, d, flow, source_b=True)[0]
    for m in (d["gt_masks"], d["gt_masks"].to(torch.uint8), d["gt_masks"].float(), d["gt_masks"].double()):
        assert torch.equal(flow_eval.filter_flow_by_mask(flow, m, INV), want)
    assert torch.equal(flow_eval.filter_flow_by_depth(flow, d["gt_depth"], d["depth"], INV, 0.2),
                       run_filter("depth_or", b, d, flow, source_b=True)[0])
    assert torch.equal(flow_eval.filter_flow_by_depth(flow, d["gt_depth"], d["depth"], INV, 0.2, "reference"),
                       flow)
    face = run_filter("face", b, d, flow, source_b=True)[0]
    assert torch.equal(flow_eval.filter_flow_by_face_index(flow, d["face_index"], d["gt_face_index"], INV), face)
    assert torch.equal(flow_eval.filter_flow_by_face_index(flow, d["face_index"].int(),
                                                           d["gt_face_index"].int(), INV), face)
    assert torch.equal(flow, keep)  # out of place
    fused = flow_eval.gt_flow(*poses(d), INV, gt_mask=d["gt_masks"], gt_depth=d["gt_depth"],
                              face_index=d["face_index"], gt_face_index=d["gt_face_index"])
    assert torch.equal(fused[0], flow)
    assert torch.equal(fused[1], run_filter("all_or", b, d, flow, source_b=False)[0])
    # a non-default depth threshold
    got = flow_eval.filter_flow_by_depth(flow, d["gt_depth"], d["depth"], INV, 0.01)
    bad, near = fr.depth_filter(flow.cpu(), b["gt_depth"], b["depth"], INV, 0.01)
    check_filtered("rect depth thr 0.01", flow, got, bad, near)


def test_flows_that_leave_the_image_and_land_on_its_edge():
    """Samples 0-3: a constant flow off each of the four sides (part of the image leaves); sample 4:
    every pixel lands exactly on the last column and row."""
    from scflow_amd import ops
    H, W = 20, 36
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32),
                            indexing="ij")
    flow = torch.zeros(5, 2, H, W)
    flow[0, 0], flow[1, 0], flow[2, 1], flow[3, 1] = 10.3, -10.3, 7.3, -7.3
    flow[4, 0], flow[4, 1] = (W - 1) - xx, (H - 1) - yy
    rng = np.random.default_rng(5)
    mask = torch.ones(5, H, W)
    depth0 = torch.full((5, H, W), 100.0)
    depth1 = torch.from_numpy(rng.uniform(90.0, 130.0, (5, H, W)).astype(np.float32))
    f1 = torch.full((5, H, W), 7, dtype=torch.int64)
    f2 = torch.from_numpy(np.where(rng.uniform(size=(5, H, W)) < 0.8, 7, 3).astype(np.int64))
    g = flow.cuda()
    for tag, kw, (bad, near) in (
            ("mask", dict(gt_mask=mask.cuda()), fr.mask_filter(flow, mask)),
            ("depth", dict(depth=depth0.cuda(), depth1=depth1.cuda()), fr.depth_filter(flow, depth1, depth0)),
            ("face", dict(face_index1=f1.cuda(), face_index2=f2.cuda()), fr.face_filter(flow, f1, f2))):
        got = ops.flow_gt(flow_in=g, invalid_num=INV, want_flow=False, **kw)[1]
        check_filtered(f"leaving {tag}", g, got, bad, near)
        out = invalid(got.cpu())
        # the columns / rows whose target is outside are invalid for every filter
        assert out[0, :, 26:].all() and out[1, :, :10].all() and out[2, 13:].all() and out[3, :7].all()
        assert not out[0].all() and not out[1].all() and not out[2].all() and not out[3].all()
        if tag == "mask":  # align_corners=False: the last pixel centre is half outside
            assert out[4].all()
        elif tag == "depth":  # the edge pixel itself is sampled: consistent where |100 − d1| < 0.2·100.1
            want = (100.0 - depth1[4, H - 1, W - 1]).abs() / 100.1 >= 0.2
            assert bool(out[4].all()) == bool(want) and bool(out[4].any()) == bool(want)
        else:
            assert bool(out[4].all()) == bool(f2[4, H - 1, W - 1] != 7)


# ------------------------------------------------------------------------------------ EPE
def epe_inputs(name):
    key = ("epe", name)
    if key not in _CACHE:
        cpu = fr.epe_case(name)
        _CACHE[key] = (cpu, tuple(t.cuda() for t in cpu))
    return _CACHE[key]


@pytest.mark.parametrize("variant", ["plain", "mask_occ", "thresholds"])
@pytest.mark.parametrize("name", fr.CASES)
def test_epe_statistics_against_the_restatement(gold, name, variant):
    from scflow_amd import flow_eval
    (tgt, pred, mask, occ), (gt, gp, gm, go) = epe_inputs(name)
    dev = gold[f"dev_{name}"]
    threshs, max_flow = ((0.5, 2.0, 4.0), 300.0) if variant == "thresholds" else ((1, 3, 5), INV)
    m_cpu, m_gpu = (None, None) if variant == "plain" else (mask, gm)
    o_cpu, o_gpu = (None, None) if variant == "plain" else (occ, go)
    want = fr.epe_stats(tgt, pred, m_cpu, max_flow, threshs, o_cpu)
    got = flow_eval.flow_stats(gt, gp, m_gpu, max_flow, threshs, o_gpu, error_map=True)
    again = flow_eval.flow_stats(gt, gp, m_gpu, max_flow, threshs, o_gpu)
    for k in ("count", "below", "err_sum") + (("occ_sum",) if o_gpu is not None else ()):
        assert torch.equal(got[k], again[k]), k  # bitwise reproducible
    assert ("occ_sum" in got) == (o_gpu is not None)
    near = want["near"]
    near_validity = ((fr.d64(tgt) ** 2).sum(1).sqrt() - max_flow).abs() < fr.NEAR_PX
    excluded = near.sum((1, 2))
    share = float(near.double().mean())
    count, below = got["count"].cpu().long(), got["below"].cpu().long()
    dcount = (count - want["count"]).abs()
    dbelow = (below - want["below"]).abs()
    tot = want["count"].double() + 1e-10
    mean_gpu = got["err_sum"].cpu() / (count.double() + 1e-10)
    dmean = (mean_gpu - want["err_sum"] / tot).abs()
    dtotal = abs(float(got["err_sum"].cpu().sum() / (count.sum().double() + 1e-10)
                       - want["err_sum"].sum() / (want["count"].sum().double() + 1e-10)))
    emap = got["error_map"].cpu().double()
    dmap = float(((emap - want["error_map"]).abs() * (~near).double()).max())
    note(f"epe {name} {variant}: near share {share:.4f}, count diff {dcount.tolist()} / below diff "
         f"{dbelow.amax(1).tolist()} (excluded {excluded.tolist()}), per-sample mean dev "
         f"{float(dmean.max()):.3e} px (gate {4 * dev[1]:.3e}), total mean dev {dtotal:.3e} px (gate "
         f"{4 * dev[0]:.3e}), map dev {dmap:.3e} px (gate {4 * dev[2]:.3e})")
    assert share <= NEAR_MAX
    assert int(near_validity.sum()) == 0  # so no flipped validity can move a sum
    assert bool((dcount <= excluded).all()) and bool((dbelow <= excluded[:, None]).all())
    assert torch.equal(count, want["count"])  # no validity is near a decision: the counts are exact
    assert float(dmean.max()) <= 4 * dev[1] and dtotal <= 4 * dev[0] and dmap <= 4 * dev[2]
    assert bool((emap[~want["valid"]] == 0).all())
    assert torch.isfinite(got["err_sum"]).all()
    if o_gpu is not None:
        docc = float(((got["occ_sum"].cpu() - want["occ_sum"]).abs() / got["num_pixels"]).max())
        note(f"epe {name} {variant}: occlusion mean dev {docc:.3e} (gate {OCC_TOL:.3e})")
        assert docc <= OCC_TOL
    empty = want["count"] == 0  # 'rect' sample 1: no depth anywhere
    assert name != "rect" or bool(empty[1])
    assert bool((got["err_sum"].cpu()[empty] == 0).all()) and bool((below[empty] == 0).all())


@pytest.mark.parametrize("name", fr.CASES)
def test_cal_epe_and_eval_epe_and_occ(gold, name):
    from scflow_amd import flow_eval
    (tgt, pred, mask, occ), (gt, gp, gm, go) = epe_inputs(name)
    dev = gold[f"dev_{name}"]
    for m_cpu, m_gpu in ((None, None), (mask, gm), (mask, gm.bool())):
        per, per_w = flow_eval.cal_epe(gt, gp, m_gpu, INV, "mean"), fr.cal_epe(tgt, pred, m_cpu, INV, "mean")
        tm, tm_w = flow_eval.cal_epe(gt, gp, m_gpu, INV, "total_mean"), fr.cal_epe(tgt, pred, m_cpu, INV, "total_mean")
        none = flow_eval.cal_epe(gt, gp, m_gpu, INV, "none")
        st = fr.epe_stats(tgt, pred, m_cpu, INV)
        assert list(per) == list(tm) == ["mean", "1px", "3px", "5px"]
        assert float((per["mean"].cpu() - per_w["mean"]).abs().max()) <= 4 * dev[1]
        assert abs(float(tm["mean"].cpu() - tm_w["mean"])) <= 4 * dev[0]
        assert torch.isfinite(per["mean"]).all() and none.shape == tgt[:, 0].shape
        assert float(((none.cpu().double() - st["error_map"]).abs() * (~st["near"]).double()).max()) <= 4 * dev[2]
        excluded = st["near"].sum((1, 2)).double()
        for t in (1, 3, 5):  # accuracies over the valid pixels: off by at most the excluded pixels
            tol = excluded / (st["count"].double() + 1e-10) + 1e-12
            assert bool(((per[f"{t}px"].cpu() - per_w[f"{t}px"]).abs() <= tol).all())
            assert abs(float(tm[f"{t}px"].cpu() - tm_w[f"{t}px"])) <= float(excluded.sum() / (st["count"].sum() + 1e-10)) + 1e-12
    # eval_epe_and_occ from the poses: its GT flows are the kernel's own (pinned above against
    # lift_points + pose_flow and, filtered, against the restatement), so restate on those.  dev is
    # the reference's deviation at this shape and error distribution (pred_flow's noise).
    b, d, flow, flow_cpu = scene(name)
    noc_cpu = flow_eval.gt_flow(*poses(d), INV, gt_mask=d["gt_masks"])[1].cpu()
    pred_g = fr.pred_flow(flow_cpu, 1)
    for masks in (d["gt_masks"], None):
        for occl in (go, None):
            got = flow_eval.eval_epe_and_occ(pred_g.cuda(), occl, d["depth"], d["gt_rotation"],
                                             d["gt_translation"], d["internel_k"], d["ref_rotation"],
                                             d["ref_translation"], masks, INV, "total_mean")
            noc = None if masks is None else noc_cpu
            want = fr.eval_epe_and_occ(pred_g, None if occl is None else occ, flow_cpu, noc, INV)
            assert list(got) == list(want), (list(got), list(want))
            for k in got:
                st = fr.epe_stats(noc_cpu if "noc" in k else flow_cpu, pred_g, None, INV)
                px = float(st["near"].sum()) / float(st["count"].sum() + 1e-10) + 1e-12
                tol = OCC_TOL if k == "occ" else 4 * dev[0] if k.endswith("mean") else px
                assert abs(float(got[k].cpu()) - float(want[k])) <= tol, (k, float(got[k]), float(want[k]))
    both = flow_eval.eval_epe_and_occ(pred_g.cuda(), None, d["depth"], d["gt_rotation"], d["gt_translation"],
                                      d["internel_k"], d["ref_rotation"], d["ref_translation"], None, INV,
                                      "total_mean", noc_without_mask=True)
    assert all(float(both[f"epe_noc_{k}"]) == float(both[f"epe_{k}"]) for k in ("mean", "1px", "3px", "5px"))


def test_wrappers_refuse_bad_gpu_arguments():
    from scflow_amd import ops
    flow = torch.zeros(2, 2, 8, 12, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        ops.flow_gt(flow_in=flow.transpose(2, 3), gt_mask=torch.ones(2, 12, 8, device="cuda"))
    with pytest.raises(ValueError, match="empty"):
        ops.flow_epe(flow[:0], flow[:0])
    with pytest.raises(TypeError):
        ops.flow_gt(flow_in=flow, gt_mask=torch.ones(2, 8, 12, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="must be"):
        ops.flow_gt(flow_in=flow, gt_mask=torch.ones(2, 8, 8, device="cuda"))
    with pytest.raises(ValueError, match="depth_combine"):
        ops.flow_gt(flow_in=flow, depth=flow[:, 0].contiguous(), depth1=flow[:, 1].contiguous(), depth_combine="and")
