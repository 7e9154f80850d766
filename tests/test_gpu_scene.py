"""GPU: ``scflow_scene_visibility`` (scflow_amd/csrc/scene.hip) against the float64 restatement
(``tests/scene_restatement.py``) on the cases of ``tests/scene_cases.py``, under its rule: a pixel
ambiguous for any instance of a frame (an edge or a decision within 64 float32 ulps of flipping) is
left out of the map comparisons for every instance of that frame and bounds the counters; every
other pixel is equal, depths within a relative 1e-5.  ``tests/test_scene_host.py`` shows on the CPU
that the cases meet the rule's condition.  Then the closed forms, reproducibility, one output at a
time, the wrapper's sort, skipped instances, untouched outputs on SCFLOW_EINVAL, ``vsd_frames`` and
the masks that ``frames_to_train_patches`` takes.

Observed on the MI355X (``profiles/scene_visib/gputest_figures.txt``): see DESIGN.md §23."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import bop_restatement as br
from tests import scene_cases as sc
from tests import scene_restatement as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = os.path.join(ROOT, "profiles", "scene_visib", "gputest_figures.txt")
ALL = ("stats", "inst_id", "depth_scene", "depth_inst", "mask_visib")


@pytest.fixture(scope="module")
def table():
    from scflow_amd import scene
    return scene.mesh_table(sc.meshes(), "cuda")


def _dev(a, dt=torch.float32):
    return None if a is None else torch.as_tensor(np.array(a)).to(dt).cuda()


def _run(table, c, want=ALL, perm=None):
    from scflow_amd import scene
    p = slice(None) if perm is None else perm
    return scene.scene_visibility(table, _dev(c["labels"][p], torch.int32), _dev(c["frame_index"][p], torch.int32),
                                  _dev(c["R"][p]), _dev(c["t"][p]), _dev(c["K"]), c["H"], c["W"],
                                  _dev(c["depth_test"]), c["delta"], c["margin"], c["pixel_offset"], want)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", sc.CASES)
def test_case_against_the_restatement(table, name):
    c = sc.case(name)
    got = _np(_run(table, c))
    fig = sc.compare(got, sc.reference(name), c)
    line = (f"{name}: ambiguous {fig['ambiguous']}, differing map pixels {fig['flips']}, largest counter "
            f"difference {fig['dstat']}, largest relative depth difference {fig['dz']:.2e}")
    print(line)
    try:
        os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
        old = [l for l in open(FIGURES).read().splitlines() if not l.startswith(name + ":")] \
            if os.path.exists(FIGURES) else []
        with open(FIGURES, "w") as f:
            f.write("\n".join(old + [line]) + "\n")
    except OSError:
        pass  # a read-only checkout: the figures are printed above


@pytest.mark.parametrize("form", sc.closed_forms(), ids=lambda f: f[0])
def test_closed_forms_are_exact(form):
    from scflow_amd import scene
    _, meshes, a, expect = form
    t = scene.mesh_table(meshes, "cuda")
    out = scene.scene_visibility(t, _dev(a["labels"], torch.int32), _dev(a["frame_index"], torch.int32),
                                 _dev(a["R"]), _dev(a["t"]), _dev(a["K"]), a["H"], a["W"], _dev(a["depth_test"]),
                                 a["delta"], a["margin"], a["pixel_offset"], ALL)
    ref = sr.scene_visibility(meshes, a["labels"], a["frame_index"], a["R"], a["t"], a["K"], a["H"], a["W"],
                              a["depth_test"], a["delta"], a["margin"], a["pixel_offset"])
    got = _np(out)
    for i, want in expect.items():
        s = sc.stats_dict(got["stats"][i])
        for k, v in want.items():
            assert s[k] == v, (i, k, s[k], v)
    assert np.array_equal(got["stats"], ref["stats"])
    assert np.array_equal(got["inst_id"], ref["inst_id"]) and np.array_equal(got["mask_visib"], ref["mask_visib"])
    assert np.array_equal(got["depth_inst"] > 0, ref["depth_inst"] > 0)
    np.testing.assert_allclose(got["depth_inst"], ref["depth_inst"], rtol=sc.EPS_Z)
    from scflow_amd.scene import visib_fract
    vf = visib_fract(out["stats"]).cpu().numpy()
    for i, want in expect.items():
        if "visib_fract" in want:
            assert vf[i] == want["visib_fract"]


@pytest.mark.parametrize("name", ("crowd", "special"))
def test_reproducible_and_one_output_at_a_time(table, name):
    c = sc.case(name)
    a, b = _run(table, c), _run(table, c)
    for k in ALL:
        assert torch.equal(a[k], b[k]), k
    for k in ALL:
        alone = _run(table, c, (k,))
        assert set(alone) == {k} and torch.equal(alone[k], a[k]), k


def test_unsorted_frame_index_through_the_wrapper(table):
    c = sc.case("crowd_dt")
    n = len(c["labels"])
    perm = np.random.default_rng(0).permutation(n)
    a, b = _run(table, c), _run(table, c, perm=perm)
    p = torch.from_numpy(perm).cuda()
    for k in ("stats", "depth_inst", "mask_visib"):
        assert torch.equal(b[k], a[k][p]), k
    assert torch.equal(b["depth_scene"], a["depth_scene"])
    inv = torch.empty(n, dtype=torch.int64, device="cuda")
    inv[p] = torch.arange(n, device="cuda")
    ida = a["inst_id"].long()
    # a tie between equal distances goes to the lower index in the order given: none in this case
    assert torch.equal(b["inst_id"].long(), torch.where(ida >= 0, inv[ida.clamp(min=0)], ida))


def test_skipped_instances_leave_zeros(table):
    c = sc.case("special")
    got = _np(_run(table, c))
    skipped = sc.reference("special")["skipped"]
    assert skipped.sum() == 3
    for i in np.nonzero(skipped)[0]:
        assert got["stats"][i].tolist() == [0, 0, 0] + [-1] * 8 + [0]
        assert not got["depth_inst"][i].any() and not got["mask_visib"][i].any()
        assert not (got["inst_id"] == i).any()
    assert (got["inst_id"][1] == -1).all() and (got["depth_scene"][1] == 0).all()   # the empty frame


def test_einval_leaves_outputs_untouched(table):
    from scflow_amd import _lib
    from tests.test_scene_host import EINVAL_CASES
    lib = _lib.load()
    c = sc.case("wide")
    n, F, H, W = len(c["labels"]), c["F"], c["H"], c["W"]
    ins = dict(labels=_dev(c["labels"], torch.int32), frame_index=_dev(c["frame_index"], torch.int32),
               R=_dev(c["R"]), t=_dev(c["t"]), K=_dev(c["K"]))
    outs = dict(stats=torch.full((n, 12), 77, dtype=torch.int32, device="cuda"),
                inst_id=torch.full((F, H, W), 77, dtype=torch.int32, device="cuda"),
                depth_scene=torch.full((F, H, W), 77.0, device="cuda"),
                depth_inst=torch.full((n, H, W), 77.0, device="cuda"),
                mask_visib=torch.full((n, H, W), 77, dtype=torch.uint8, device="cuda"))

    def args(**kw):
        a = _lib.SceneArgs()
        for k in ("verts", "faces", "vert_offset", "face_offset", "bounds"):
            setattr(a, k, getattr(table, k).data_ptr())
        a.num_classes, a.total_verts, a.total_faces = table.num_classes, table.verts.shape[0], table.faces.shape[0]
        for k, v in list(ins.items()) + list(outs.items()):
            setattr(a, k, v.data_ptr())
        a.n, a.n_frames, a.height, a.width, a.margin_x, a.margin_y = n, F, H, W, 0, 0
        a.pixel_offset, a.delta = 0.0, 15.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    stream = torch.cuda.current_stream().cuda_stream
    none = dict(stats=None, inst_id=None, depth_scene=None, depth_inst=None, mask_visib=None)
    for kw in [k for k in EINVAL_CASES if k != dict(stats=None)] + [none]:
        assert lib.scflow_scene_visibility(ctypes.byref(args(**kw)), stream) == -1, kw
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == 77).all()), k


def test_vsd_frames_equals_vsd_counts_on_the_restated_planes(table):
    """48×64 frames; the pixels whose count membership is within the float32 tolerances of a
    threshold are ambiguous (``bop_restatement.vsd_counts``' rule) and bound the differences."""
    from scflow_amd import bop_metrics as bm
    c = sc.case("special")
    keep = ~sc.reference("special")["skipped"]
    lab, fi, R, t = (c[k][keep] for k in ("labels", "frame_index", "R", "t"))
    rng = np.random.default_rng(3)
    t_est = (t + rng.normal(0, 4.0, t.shape)).astype(np.float32)
    Kp = c["K"][fi]
    diam = np.full(len(lab), 110.0, np.float32)
    e = bm.vsd_frames(table, _dev(lab, torch.int32), _dev(R), _dev(t_est), _dev(R), _dev(t), _dev(Kp),
                      _dev(c["depth_test"]), _dev(fi, torch.int32), _dev(diam)).cpu().numpy()
    r_est = sr.scene_visibility(sc.meshes(), lab, fi, R, t_est, c["K"], c["H"], c["W"])
    r_gt = sr.scene_visibility(sc.meshes(), lab, fi, R, t, c["K"], c["H"], c["W"])
    for i in range(len(lab)):
        counts, amb, _ = br.vsd_counts(r_est["depth_inst"][i], r_gt["depth_inst"][i], c["depth_test"][fi[i]],
                                       Kp[i], bm.BOP19_DELTA, bm.BOP19_TAUS, float(diam[i]))
        f = int(fi[i])
        edge = ((r_est["edge_margin"][i] < r_est["edge_thr"][i]) | (r_gt["edge_margin"][i] < r_gt["edge_thr"][i]))
        slack = int(amb) + int(edge.sum())
        want = br.vsd_errors(counts)
        u = max(int(counts[0]), 1)
        assert np.all(np.abs(e[i] - want) <= 2.0 * slack / u + 1e-12), (i, f, e[i], want, slack)


def test_foreground_masks_feed_the_training_patches(table):
    from scflow_amd import patches, scene
    c = sc.case("wide")
    ref = sc.reference("wide")
    out = _run(table, c, ("inst_id",))
    fg = scene.foreground_masks(out["inst_id"])
    fg_ref = torch.from_numpy((ref["inst_id"] >= 0).astype(np.uint8)).cuda()
    amb_f, _ = sr.ambiguous(ref, c["frame_index"], c["F"], c["margin"])
    # the masks agree outside the ambiguous pixels; where none is ambiguous the batches are equal
    assert torch.equal(fg[~torch.from_numpy(amb_f).cuda()], fg_ref[~torch.from_numpy(amb_f).cuda()])
    fg_same = torch.where(torch.from_numpy(amb_f).cuda(), fg_ref, fg)
    m = sc.meshes()

    class R:
        meshes = {l: (torch.from_numpy(np.array(v)).cuda(),) for l, (v, f) in m.items()}
    points, counts = patches.point_table(R())
    F, H, W = c["F"], c["H"], c["W"]
    frames = torch.randint(0, 255, (F, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    diam = torch.full((points.shape[0],), 110.0, device="cuda")
    kw = dict(seed=5, step=0, size=32)
    call = lambda masks: patches.frames_to_train_patches(  # noqa: E731
        frames, masks, _dev(c["frame_index"], torch.int32), _dev(c["R"]), _dev(c["t"]), _dev(c["K"]),
        _dev(c["labels"], torch.int64), points, counts, diam, **kw)
    a, b = call(fg_same), call(fg_ref)
    assert torch.equal(a["gt_masks"], b["gt_masks"]) and a["gt_masks"].sum() > 0
    assert torch.equal(a["real_images"], b["real_images"])
