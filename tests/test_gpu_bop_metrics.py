"""GPU: the BOP pose-error kernels (``scflow_pose_err_sym``, ``scflow_vsd_counts``) and
``scflow_amd.bop_metrics`` against the float64 restatement (tests/bop_restatement.py) on the shared
seeded cases (tests/bop_cases.py).

MSSD / MSPD bounds, from fp32 ulps at the cases' magnitudes (t_z ≤ 1500, ‖x‖ ≤ 139, |u| ≤ ~700):
MSSD ≤ 32·2⁻²³·(max |t| + max ‖x‖) ≈ 6e-3, MSPD ≤ 64·2⁻²³·max(|u|, |v|, W) ≈ 6e-3 px; an fp32 numpy
evaluation differs from fp64 by about 1e-4 on such inputs, so the bounds leave room for another
operation order and none for a wrong vertex or symmetry.  VSD counts are integers: each may
differ from the restatement's by at most the case's number of ambiguous pixels (decisions whose
margin is below 64 fp32 ulps of the largest distance; ≤ 1 % of the union for every case, asserted
on the CPU in tests/test_bop_metrics_host.py) and is equal where that number is 0.  Observed
maxima: DESIGN.md §22."""
import numpy as np
import pytest
import torch

from scflow_amd import _lib, bop_metrics as bm
from scflow_amd._lib import ScflowError
from scflow_amd.renderer import Renderer
from tests import bop_cases as bc
from tests import bop_restatement as br

pytestmark = pytest.mark.gpu

DEV = "cuda"


def T(a, dt=torch.float32):
    return torch.from_numpy(np.array(a)).to(dt).to(DEV)   # a copy: the shared cases are read-only


@pytest.fixture(scope="module")
def table():
    points, counts, info, kinds = bc.classes()
    sym, off = bm.symmetry_table(info, len(kinds), DEV)
    return dict(points=T(points), counts=T(counts, torch.int32), sym=sym, off=off, info=info, kinds=kinds)


def _poses(b):
    return [T(b[k]) for k in ("R_est", "t_est", "R_gt", "t_gt")]


def _run(table, b, which="both"):
    s, p = bm.mssd_mspd(table["points"], table["counts"], table["sym"], table["off"],
                        T(b["labels"], torch.int64), *_poses(b), T(b["K"]), which=which)
    return s, p


# ------------------------------------------------------------------------------ MSSD / MSPD
def test_symmetry_table_is_the_restatement_packed(table):
    off = table["off"].cpu().numpy()
    sym = table["sym"].cpu().numpy()
    assert off[0] == 0 and off[-1] == sym.shape[0] and sym.shape[1] == 12
    for c, (_, s) in enumerate(table["kinds"]):
        ref = br.symmetry_set(table["info"][str(c + 1)])
        assert off[c + 1] - off[c] == len(ref) == s
        for row, (R, t) in zip(sym[off[c]:off[c + 1]], ref):
            # two float64 evaluations rounded to float32: an ulp of the largest entry (< 16)
            assert np.abs(row.reshape(3, 4) - np.hstack([R, t[:, None]])).max() <= 2.0 ** -19


@pytest.mark.parametrize("n", [1, 70])
def test_mssd_mspd_against_the_restatement(table, n):
    b = bc.pose_batch(n)
    ref_s, ref_p, tol_s, tol_p = bc.pose_reference(n)
    s, p = _run(table, b)
    s2, p2 = _run(table, b)
    torch.cuda.synchronize()
    s_, p_ = s.double().cpu().numpy(), p.double().cpu().numpy()
    empty = np.isinf(ref_s)
    assert empty.sum() == (4 if n == 70 else 0)       # the class without vertices → +inf
    assert np.array_equal(np.isinf(s_), empty) and np.array_equal(np.isinf(p_), empty)
    ds, dp = np.abs(s_[~empty] - ref_s[~empty]).max(), np.abs(p_[~empty] - ref_p[~empty]).max()
    print(f"n={n}: max |MSSD − ref| {ds:.3e} (bound {tol_s:.3e}), max |MSPD − ref| {dp:.3e} px (bound {tol_p:.3e})")
    assert ds <= tol_s and dp <= tol_p
    assert torch.equal(s, s2) and torch.equal(p, p2)          # run to run: bitwise
    s_alone, none = _run(table, b, "mssd")
    assert none is None and torch.equal(s_alone, s)            # alone = joint: bitwise
    none, p_alone = _run(table, b, "mspd")
    assert none is None and torch.equal(p_alone, p)


def test_mssd_without_k_and_mspd_needs_k(table):
    b = bc.pose_batch(70)
    s, p = bm.mssd_mspd(table["points"], table["counts"], table["sym"], table["off"],
                        T(b["labels"], torch.int64), *_poses(b))
    assert p is None and torch.equal(s, _run(table, b)[0])
    with pytest.raises(ScflowError):
        bm.mssd_mspd(table["points"], table["counts"], table["sym"], table["off"],
                     T(b["labels"], torch.int64), *_poses(b), which="mspd")


def test_mssd_of_the_identity_set_is_the_largest_point_distance(table):
    """With S = {identity}, MSSD is the max over the points of the distances whose MEAN
    ``metrics.pose_errors`` reports as ADD: the same distances by torch on the device."""
    b = bc.pose_batch(70)
    s, _ = _run(table, b)
    _, _, tol_s, _ = bc.pose_reference(70)
    Re, te, Rg, tg = _poses(b)
    checked = 0
    for i, lab in enumerate(b["labels"]):
        P, S = table["kinds"][lab]
        if S != 1 or P == 0:
            continue
        pts = table["points"][lab, :P]
        d = ((pts @ Re[i].T + te[i]) - (pts @ Rg[i].T + tg[i])).norm(dim=-1)
        assert abs(float(d.max()) - float(s[i])) <= tol_s, (i, lab)
        checked += 1
    assert checked >= 12


def _raw_pose_err(table, b, **override):
    """scflow_pose_err_sym through ctypes with outputs pre-filled with 7; returns (rc, mssd, mspd)."""
    n = len(b["labels"])
    t = dict(points=table["points"], counts=table["counts"], sym=table["sym"], off=table["off"],
             labels=T(b["labels"], torch.int32), K=T(b["K"]))
    t.update(zip(("Re", "te", "Rg", "tg"), _poses(b)))
    s, p = torch.full((n,), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)
    a = dict(points=t["points"].data_ptr(), counts=t["counts"].data_ptr(), C=t["points"].shape[0],
             P=t["points"].shape[1], sym=t["sym"].data_ptr(), off=t["off"].data_ptr(), total=t["sym"].shape[0],
             labels=t["labels"].data_ptr(), Re=t["Re"].data_ptr(), te=t["te"].data_ptr(), Rg=t["Rg"].data_ptr(),
             tg=t["tg"].data_ptr(), K=t["K"].data_ptr(), mssd=s.data_ptr(), mspd=p.data_ptr(), n=n)
    a.update(override)
    rc = _lib.load().scflow_pose_err_sym(*a.values(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, s.cpu().numpy(), p.cpu().numpy()


def test_pose_err_refuses_bad_arguments_and_leaves_the_outputs(table):
    b = bc.pose_batch(70)
    bad = [dict(points=None), dict(counts=None), dict(sym=None), dict(off=None), dict(labels=None),
           dict(Re=None), dict(te=None), dict(Rg=None), dict(tg=None), dict(K=None),
           dict(mssd=None, mspd=None), dict(C=0), dict(P=0), dict(total=0), dict(n=-1)]
    for o in bad:
        rc, s, p = _raw_pose_err(table, b, **o)
        assert rc == -1, o
        assert (s == 7.0).all() and (p == 7.0).all(), o
    rc, s, p = _raw_pose_err(table, b, n=0)       # a no-op success
    assert rc == 0 and (s == 7.0).all() and (p == 7.0).all()
    rc, s, p = _raw_pose_err(table, b, K=None, mspd=None)   # MSSD alone needs no K
    assert rc == 0 and (p == 7.0).all() and not (s == 7.0).any()


def test_labels_outside_the_table_stay_infinite(table):
    b = dict(bc.pose_batch(70))
    lab = np.array(b["labels"])
    lab[3], lab[5] = -1, len(table["kinds"])
    lab_dev = T(lab, torch.int32)
    rc, s, p = _raw_pose_err(table, b, labels=lab_dev.data_ptr())
    assert rc == 0 and np.isinf(s[[3, 5]]).all() and np.isinf(p[[3, 5]]).all()
    assert np.isfinite(s[[0, 1, 2, 4]]).all()


# ------------------------------------------------------------------------------ VSD counts
def _counts(c, **kw):
    return bm.vsd_counts(T(c["depth_est"]), T(c["depth_gt"]), T(c["depth_test"]), T(c["frame_index"], torch.int32),
                         T(c["K"]), None if c["diameter"] is None else T(c["diameter"]), c["taus"], bc.DELTA, **kw)


@pytest.mark.parametrize("case", bc.vsd_case_list(), ids=lambda c: "{}x{}-n{}-t{}-{}-f{}".format(
    c[0], c[1], c[2], c[3], "diam" if c[4] else "mm", c[5]))
def test_vsd_counts_against_the_restatement(case):
    c = bc.vsd_case(*case)
    ref, amb = bc.vsd_reference(*case)
    got = _counts(c)
    again = _counts(c)
    torch.cuda.synchronize()
    g = got.cpu().numpy().astype(np.int64)
    assert g.shape == ref.shape and got.dtype == torch.int32
    diff = int(np.abs(g - ref).max())
    print(f"{case}: union {int(ref[:, 0].sum())}, ambiguous {amb}, max count difference {diff}")
    assert np.abs(g - ref).sum(0).max() <= amb      # per counter, over the case: ≤ the ambiguous pixels
    if amb == 0:
        assert np.array_equal(g, ref)
    assert torch.equal(got, again)
    assert (g[:, 1] <= g[:, 0]).all() and (g[:, 2:] <= g[:, 1:2]).all()


def test_vsd_closed_forms_on_the_kernel():
    c = bc.vsd_case(33, 65, 6, 10, True, 3)
    gt = T(c["depth_gt"])
    fi = torch.arange(6, dtype=torch.int32, device=DEV)
    K, d = T(c["K"]), T(c["diameter"])
    mask = (gt > 0).sum((1, 2)).int()
    # est = GT, test = the GT depth: |U| = |I| = the mask, no cost, errors exactly 0
    k = bm.vsd_counts(gt, gt, gt, fi, K, d)
    assert torch.equal(k[:, 0], mask) and torch.equal(k[:, 1], mask) and not k[:, 2:].any()
    assert torch.equal(bm.vsd_errors(k), torch.zeros(6, 10, dtype=torch.float64, device=DEV))
    # an empty estimate (0, and the renderer's −1): |I| = 0, errors exactly 1
    for empty in (torch.zeros_like(gt), torch.full_like(gt, -1.0)):
        k = bm.vsd_counts(empty, gt, gt, fi, K, d)
        assert torch.equal(k[:, 0], mask) and not k[:, 1:].any()
        assert torch.equal(bm.vsd_errors(k), torch.ones(6, 10, dtype=torch.float64, device=DEV))
    # an occluder nearer than δ everywhere: |U| = 0, errors exactly 1
    k = bm.vsd_counts(gt, gt, torch.full_like(gt, 300.0), fi, K, d)
    assert not k.any() and torch.equal(bm.vsd_errors(k), torch.ones(6, 10, dtype=torch.float64, device=DEV))
    # no test depth at all: every rendered pixel is visible
    est = T(c["depth_est"])
    k = bm.vsd_counts(est, gt, torch.zeros_like(gt), fi, K, d)
    assert torch.equal(k[:, 0], ((gt > 0) | (est > 0)).sum((1, 2)).int())
    assert torch.equal(k[:, 1], ((gt > 0) & (est > 0)).sum((1, 2)).int())


def test_vsd_counts_refuses_bad_arguments_and_leaves_counts():
    c = bc.vsd_case(5, 7, 6, 10, True, 3)
    t = dict(est=T(c["depth_est"]), gt=T(c["depth_gt"]), test=T(c["depth_test"]),
             fi=T(c["frame_index"], torch.int32), K=T(c["K"]), diam=T(c["diameter"]), taus=T(np.array(c["taus"])))
    lib = _lib.load()

    def call(**o):
        counts = torch.full((6, 12), 7, dtype=torch.int32, device=DEV)
        a = dict(est=t["est"].data_ptr(), gt=t["gt"].data_ptr(), test=t["test"].data_ptr(), fi=t["fi"].data_ptr(),
                 K=t["K"].data_ptr(), diam=t["diam"].data_ptr(), taus=t["taus"].data_ptr(), n_taus=10,
                 delta=15.0, counts=counts.data_ptr(), n=6, frames=2, h=5, w=7)
        a.update(o)
        if a["counts"] is None:
            return lib.scflow_vsd_counts(*a.values(), torch.cuda.current_stream().cuda_stream), counts
        rc = lib.scflow_vsd_counts(*a.values(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, counts
    for o in (dict(est=None), dict(gt=None), dict(test=None), dict(fi=None), dict(K=None), dict(taus=None),
              dict(counts=None), dict(n=-1), dict(frames=0), dict(h=0), dict(w=0), dict(n_taus=0), dict(n_taus=17)):
        rc, counts = call(**o)
        assert rc == -1, o
        assert (counts == 7).all(), o
    rc, counts = call(n=0)
    assert rc == 0 and (counts == 7).all()
    rc, counts = call(diam=None)               # NULL diameter is the not-normalised mode
    assert rc == 0 and not (counts == 7).all()
    # a frame index outside the frames leaves that pair's counts 0
    fi = T(np.array([0, 0, 0, 1, 2, -1]), torch.int32)
    rc, counts = call(fi=fi.data_ptr())
    assert rc == 0 and not counts[4:].any() and int(counts[:4, 0].sum()) > 0


# ------------------------------------------------------------------------------ vsd via Renderer
@pytest.fixture(scope="module")
def scene():
    c = bc.ar_case()
    r = Renderer(image_size=(bc.AR_SIZE, bc.AR_SIZE), soft_blending=False, render_mask=False,
                 render_image=False, meshes={i: tuple(np.array(x) for x in m) for i, m in c["meshes"].items()}).to(DEV)
    lab = T(c["labels"], torch.int64)
    K = T(c["K"])
    z_est = r(T(c["R_est"]), T(c["t_est"]), K, lab)["fragments"].zbuf[..., 0]
    z_gt = r(T(c["R_gt"]), T(c["t_gt"]), K, lab)["fragments"].zbuf[..., 0]
    zg = z_gt.cpu().numpy()
    return dict(c=c, r=r, lab=lab, K=K, z_est=z_est.cpu().numpy(), z_gt=zg, test=bc.ar_test_depth(zg))


def _restated_vsd(s, rows=bc.AR_SIZE):
    return bc.ar_vsd_reference(s["z_est"], s["z_gt"], s["test"], rows)


def _vsd(s, test, renderer=None):
    c = s["c"]
    return bm.vsd(renderer or s["r"], s["lab"], T(c["R_est"]), T(c["t_est"]), T(c["R_gt"]), T(c["t_gt"]), s["K"],
                  test, torch.arange(8, dtype=torch.int32, device=DEV), T(c["diameters"]))


@pytest.mark.parametrize("rows", [64, 48])
def test_vsd_through_the_renderer(scene, rows):
    """``vsd`` = the restatement on the renderer's own zbuf (the rasteriser's edge decisions do not
    enter); a 48-row frame reads rows [:48] of the 64² render."""
    e = _vsd(scene, T(scene["test"][:, :rows]))
    assert e.shape == (8, 10) and e.dtype == torch.float64
    counts, amb = _restated_vsd(scene, rows)
    ref = br.vsd_errors(counts)
    union = counts[:, 0]
    assert (union > 200).all()
    d = np.abs(e.cpu().numpy() - ref)
    print(f"rows {rows}: union {union.tolist()}, ambiguous {amb.tolist()}, max |e − ref| {d.max():.3e}")
    assert (d <= (2.0 * amb / union)[:, None] + 1e-15).all()
    assert ref.min() < 0.2 and ref.max() > 0.8        # the perturbations span the range


def test_vsd_of_the_ground_truth_render_is_zero(scene):
    c = scene["c"]
    gt = [T(c["R_gt"]), T(c["t_gt"])]
    e = bm.vsd(scene["r"], scene["lab"], *gt, *gt, scene["K"], T(scene["z_gt"]),
               torch.arange(8, dtype=torch.int32, device=DEV), T(c["diameters"]))
    assert torch.equal(e, torch.zeros(8, 10, dtype=torch.float64, device=DEV))


def test_vsd_needs_a_renderer_as_large_as_the_frame(scene):
    small = Renderer(image_size=(32, 32), soft_blending=False, render_mask=False, render_image=False,
                     meshes={i: tuple(np.array(x) for x in m) for i, m in scene["c"]["meshes"].items()}).to(DEV)
    with pytest.raises(ScflowError, match="renderer"):
        _vsd(scene, T(scene["test"][:, :48]), small)


# ------------------------------------------------------------------------------ average recall
def test_average_recall_end_to_end(scene):
    """Device errors → ``average_recall`` = the restatement's errors → its own recall loops.  The
    perturbations keep every error away from every threshold (MSSD / MSPD: asserted on the CPU in
    test_bop_metrics_host.py; VSD: asserted here, on this renderer's depth)."""
    from scflow_amd.patches import point_table
    c = scene["c"]
    points, counts = point_table(scene["r"])
    info = {str(i + 1): {"diameter": float(c["diameters"][i])} for i in range(8)}
    sym, off = bm.symmetry_table(info, 8, DEV)
    assert sym.shape == (8, 12)
    s, p = bm.mssd_mspd(points, counts, sym, off, scene["lab"], T(c["R_est"]), T(c["t_est"]), T(c["R_gt"]),
                        T(c["t_gt"]), scene["K"])
    e = _vsd(scene, T(scene["test"]))
    ref_s, ref_p = bc.ar_reference()
    kc, amb = _restated_vsd(scene)
    ref_e = br.vsd_errors(kc)
    # without ambiguous pixels the counts, and so the errors, are the restatement's exactly; an
    # ambiguous pixel moves an error by at most 2 / |U|
    slack = 2.0 * amb / kc[:, 0]
    margin = bc.vsd_threshold_margins(kc)
    print("VSD margins", margin, "slack", slack)
    assert (margin > slack)[amb > 0].all()
    targets = np.array([True] * 7 + [False])
    got = bm.average_recall(e.cpu().numpy(), s.double().cpu().numpy(), p.double().cpu().numpy(),
                            c["diameters"], bc.AR_SIZE, targets)
    ref = br.average_recall(ref_e, ref_s, ref_p, c["diameters"], bc.AR_SIZE, targets)
    print({k: got[k] for k in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD")})
    for k in ("recall_vsd", "recall_mssd", "recall_mspd"):
        assert np.array_equal(got[k], ref[k]), k
    for k in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD"):
        assert got[k] == pytest.approx(ref[k], abs=1e-12)
    assert 0.0 < got["AR_MSSD"] < 1.0 and 0.0 < got["AR_MSPD"] < 1.0 and 0.0 < got["AR_VSD"] < 1.0


def test_evaluate_bop_on_the_device(scene):
    """``bop_eval.evaluate_bop`` with its own (device) error functions on the same eight objects,
    one per image, against the restatement's recalls."""
    from scflow_amd import bop_eval
    c = scene["c"]
    seq = "000001"
    pose, cam, results = {}, {}, []
    for i in range(8):
        pose[str(i)] = [dict(obj_id=i + 1, cam_R_m2c=c["R_gt"][i].reshape(-1).tolist(),
                             cam_t_m2c=c["t_gt"][i].tolist())]
        cam[str(i)] = dict(cam_K=c["K"][i].reshape(-1).tolist())
        results.append(dict(img_metas=dict(img_path=f"data/{seq}/rgb/{i:06d}.png"),
                            pred=dict(labels=np.array([i]), rotations=c["R_est"][i][None],
                                      translations=c["t_est"][i][None])))
    info = {str(i + 1): {"diameter": float(c["diameters"][i])} for i in range(8)}
    names = [f"obj_{i + 1}" for i in range(8)]
    out = bop_eval.evaluate_bop(results, {seq: dict(pose=pose, camera=cam)}, info, scene["r"],
                                lambda s, i: scene["test"][i], class_names=names)
    ref_s, ref_p = bc.ar_reference()
    ref = br.average_recall(br.vsd_errors(_restated_vsd(scene)[0]), ref_s, ref_p, c["diameters"], bc.AR_SIZE,
                            np.ones(8, bool))
    for k in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD"):
        assert out[f"all/{k}"] == pytest.approx(ref[k], abs=1e-12), k
    assert [out["all/mssd_{:02d}".format(5 * k)] for k in range(1, 11)] == ref["recall_mssd"].tolist()
    assert [out["all/mspd_{:02d}".format(5 * k)] for k in range(1, 11)] == ref["recall_mspd"].tolist()
    assert out["obj_1/AR"] == 1.0 and out["obj_8/AR"] == 0.0
