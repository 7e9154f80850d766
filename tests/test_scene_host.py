"""CPU: scene visibility's host side (``scflow_amd.scene``, ``bop_eval.compute_gt_info`` /
``write_gt_info``), the float64 restatement the GPU tests compare the kernel with
(``tests/scene_restatement.py``) on closed forms, and the condition those tests lean on: in every
committed case the ambiguous pixels are at most max(2, 1 %) of the frame's union of silhouettes,
and a float32 run of the restatement differs from the float64 run only there.

Figures of the committed cases (float32 stand-in against float64; printed by
``test_cases_are_well_conditioned``): at most 17 ambiguous pixels per frame (that frame's union is
3 072 pixels, its cap 30), no pixel of any map and no counter different, largest relative depth
difference 5.3e-6."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from scflow_amd import _lib, bop_eval, scene
from tests import helpers
from tests import scene_cases as sc
from tests import scene_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("form", sc.closed_forms(), ids=lambda f: f[0])
def test_restatement_closed_forms(form):
    _, meshes, a, expect = form
    res = sr.scene_visibility(meshes, a["labels"], a["frame_index"], a["R"], a["t"], a["K"], a["H"], a["W"],
                              a["depth_test"], a["delta"], a["margin"], a["pixel_offset"])
    for i, want in expect.items():
        got = sc.stats_dict(res["stats"][i])
        for k, v in want.items():
            assert got[k] == v, (i, k, got[k], v)
    # the far square is 500 mm deep wherever it is; inst_id names the nearest visible instance
    d = res["depth_inst"][0]
    assert np.allclose(d[d > 0], 500.0, rtol=1e-12)
    if form[0] == "half_hidden":
        assert (res["inst_id"][0, 6:16, 10:15] == 1).all() and (res["inst_id"][0, 8:15, 15:20] == 0).all()
        assert (res["inst_id"][0] >= 0).sum() == 85
        assert np.allclose(res["depth_scene"][0, 6:16, 10:15], 400.0) and res["depth_scene"][0, 0, 0] == 0
    if form[0] == "sensor_zeros":
        assert (res["mask_visib"][0] > 0).sum() == 70


@pytest.mark.parametrize("name", sc.CASES)
def test_cases_are_well_conditioned(name):
    c = sc.case(name)
    ref, f32 = sc.reference(name), sc.reference(name, fp32=True)
    amb_f, amb_c = sr.ambiguous(ref, np.clip(c["frame_index"], 0, c["F"] - 1), c["F"], c["margin"])
    for f in range(c["F"]):
        mine = [i for i in range(len(c["labels"])) if c["frame_index"][i] == f and not ref["skipped"][i]]
        union = int(ref["cover_canvas"][mine].any(0).sum()) if mine else 0
        print(f"{name}[{f}]: {len(mine)} instances, union {union}, ambiguous {int(amb_c[f].sum())}")
        assert amb_c[f].sum() <= max(2, 0.01 * union)
    got = {k: np.asarray(f32[k]) for k in ("stats", "inst_id", "depth_scene", "depth_inst", "mask_visib")}
    fig = sc.compare(got, ref, c)
    print(f"{name}: float32 against float64: {fig}")


def test_cases_have_their_properties():
    ref, c = sc.reference("special"), sc.case("special")
    s = ref["stats"]
    assert s[0, 0] == 0 and s[0, 3:7].tolist() == [-1] * 4                  # wholly outside
    assert s[1, 0] > s[1, 1] > 0 and s[1, 3] < 0 and s[1, 4] < 0            # across left and top, on the margin
    assert 0 < s[2, 0]                                                      # the faces in front are drawn
    assert s[4, 2] > 0 and s[5, 2] == s[4, 2]                               # a duplicate: both visible …
    assert not (ref["inst_id"] == 5).any() and (ref["inst_id"] == 4).any()  # … the lower index is named
    assert ref["skipped"].tolist()[-6:] == [False, False, False, True, True, True]
    crowd = sc.case("crowd")
    assert np.bincount(crowd["frame_index"]).tolist() == [40, 24, 6] and len(crowd["labels"]) == 70
    assert (sc.reference("crowd")["mask_visib"].reshape(70, -1).sum(1) == 0).any()  # someone is hidden
    assert len(sc.meshes()[3][1]) == 576
    dt = sc.reference("special")
    assert (dt["stats"][:, 1] < dt["stats"][:, 0]).any()                    # sensor zeros: not valid


# ------------------------------------------------------------------------------ host logic
def test_mesh_table_offsets_with_a_missing_class():
    t = scene.mesh_table(sc.meshes(), "cpu")
    m = sc.meshes()
    nv = [len(m[l][0]) if l in m else 0 for l in range(7)]
    nf = [len(m[l][1]) if l in m else 0 for l in range(7)]
    assert t.vert_offset.tolist() == np.concatenate([[0], np.cumsum(nv)]).tolist()
    assert t.face_offset.tolist() == np.concatenate([[0], np.cumsum(nf)]).tolist()
    assert t.vert_offset[5] == t.vert_offset[6] and t.face_offset[5] == t.face_offset[6]
    assert t.verts.dtype == torch.float32 and t.faces.dtype == torch.int32 and t.vert_offset.dtype == torch.int32
    assert t.num_classes == 7 and tuple(t.bounds.shape) == (7, 6)
    o = int(t.vert_offset[3])
    assert torch.equal(t.verts[o:o + nv[3]], torch.from_numpy(np.array(m[3][0])))
    assert int(t.faces.max()) == max(nv) - 1 and int(t.faces.min()) == 0      # local indices
    assert np.allclose(t.bounds[0].numpy(), [-45, -35, -25, 45, 35, 25])

    class R:
        meshes = {l: (torch.from_numpy(np.array(v)), torch.from_numpy(np.array(f))) for l, (v, f) in m.items()}
    t2 = scene.mesh_table(R())
    assert torch.equal(t2.faces, t.faces) and torch.equal(t2.verts, t.verts)


def test_visib_fract_and_foreground():
    s = torch.zeros(3, 12, dtype=torch.int32)
    s[0, 0], s[0, 2] = 3, 1
    s[2, 0], s[2, 2] = 7, 7
    v = scene.visib_fract(s)
    assert v.dtype == torch.float64 and v.tolist() == [1 / 3, 0.0, 1.0]
    fg = scene.foreground_masks(torch.tensor([[[-1, 0], [3, -1]]], dtype=torch.int32))
    assert fg.dtype == torch.uint8 and fg.tolist() == [[[0, 1], [1, 0]]]


class _Meshes:
    """What compute_gt_info and evaluate_bop read of a Renderer."""
    def __init__(self, meshes):
        self.meshes = {l: (torch.from_numpy(np.array(v)), torch.from_numpy(np.array(f))) for l, (v, f) in meshes.items()}
        self.image_size = (480, 640)


def _restated_stats(table, labels, frame_index, R, t, K, H, W, depth_test, delta, margin):
    out = np.zeros((len(labels), 12), np.int32)
    for f in range(len(K)):                     # frame by frame: the canvas arrays stay small
        sel = np.nonzero(frame_index == f)[0]
        res = sr.scene_visibility(table, labels[sel], np.zeros(len(sel), np.int32), R[sel], t[sel], K[f:f + 1],
                                  H, W, None if depth_test is None else depth_test[f:f + 1], delta, margin)
        out[sel] = res["stats"]
    return out


def test_compute_and_write_gt_info(tmp_path):
    helpers.make_bop_case(str(tmp_path))
    data = str(tmp_path / "data")
    ann = bop_eval.load_bop_annotations(data, ["000048", "000055"])
    box = sc.meshes()[0]
    rend = _Meshes({l: box for l in range(21)})
    # image 1 of sequence 48: the second object behind the first one on the same ray, hidden
    objs = ann["000048"]["pose"]["1"]
    objs[1]["cam_R_m2c"] = objs[0]["cam_R_m2c"]
    objs[1]["cam_t_m2c"] = (np.asarray(objs[0]["cam_t_m2c"]) * 1.5).tolist()
    bop_eval.compute_gt_info(ann, rend, None, margin=(8, 8), visibility_fn=_restated_stats)
    for seq in ann:
        assert set(ann[seq]["gt_info"]) == set(ann[seq]["pose"])
        for img, rows in ann[seq]["gt_info"].items():
            assert len(rows) == len(ann[seq]["pose"][img])
            for r in rows:
                assert set(r) == set(bop_eval.GT_INFO_KEYS)
                assert r["px_count_all"] >= r["px_count_valid"] >= r["px_count_visib"] >= 0
                assert r["visib_fract"] == (r["px_count_visib"] / r["px_count_all"] if r["px_count_all"] else 0.0)
    info = ann["000048"]["gt_info"]["1"]
    assert info[0]["visib_fract"] > 0.9 and info[1]["visib_fract"] < 0.1 and info[1]["px_count_all"] > 0
    assert info[1]["bbox_visib"] == [-1, -1, -1, -1] or info[1]["px_count_visib"] > 0
    paths = bop_eval.write_gt_info(data, ann)
    assert sorted(os.path.basename(os.path.dirname(p)) for p in paths) == ["000048", "000055"]
    back = bop_eval.load_bop_annotations(data, ["000048", "000055"])
    assert back["000048"]["gt_info"] == json.loads(json.dumps(ann["000048"]["gt_info"]))
    assert back["000055"]["gt_info"] == ann["000055"]["gt_info"]

    # evaluate_bop: every GT but the hidden one has its own pose as the estimate; the hidden one has
    # none.  With the computed gt_info it is no target and the recall is 1; without it, it counts.
    results = []
    for seq in ("000048", "000055"):
        for img, objs in back[seq]["pose"].items():
            keep = [o for k, o in enumerate(objs) if not (seq == "000048" and img == "1" and k == 1)]
            results.append(dict(img_metas=dict(img_path=f"{data}/{seq}/rgb/{int(img):06d}.png"),
                                pred=dict(labels=np.array([o["obj_id"] - 1 for o in keep]),
                                          rotations=np.array([o["cam_R_m2c"] for o in keep], np.float32).reshape(-1, 3, 3),
                                          translations=np.array([o["cam_t_m2c"] for o in keep], np.float32))))
    info_json = {str(l + 1): {"diameter": 100.0} for l in range(21)}
    zero = lambda batch, renderer: (np.zeros((len(batch["labels"]), len(batch["taus"]))),  # noqa: E731
                                    np.zeros(len(batch["labels"])), np.zeros(len(batch["labels"])))
    depth = lambda s, i: np.zeros((480, 640), np.float32)  # noqa: E731
    out = bop_eval.evaluate_bop(results, back, info_json, rend, depth, error_fn=zero)
    assert out["all/AR"] == 1.0
    bare = {s: {k: v for k, v in a.items() if k != "gt_info"} for s, a in back.items()}
    assert bop_eval.evaluate_bop(results, bare, info_json, rend, depth, error_fn=zero)["all/AR"] < 1.0


# ------------------------------------------------------------------------------ the C entry
def _args(**kw):
    """Arguments that pass every check, with made-up addresses: used only with one field broken, so
    that the call returns before any launch."""
    a = _lib.SceneArgs()
    for name in ("verts", "faces", "vert_offset", "face_offset", "bounds", "labels", "frame_index", "R", "t",
                 "K", "stats"):
        setattr(a, name, 4096)
    a.num_classes, a.total_verts, a.total_faces = 2, 8, 12
    a.n, a.n_frames, a.height, a.width, a.margin_x, a.margin_y = 3, 1, 8, 8, 0, 0
    a.pixel_offset, a.delta = 0.0, 15.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


EINVAL_CASES = [dict(verts=None), dict(faces=None), dict(vert_offset=None), dict(face_offset=None),
                dict(bounds=None), dict(labels=None), dict(frame_index=None), dict(R=None), dict(t=None),
                dict(K=None), dict(num_classes=0), dict(total_verts=0), dict(total_faces=0), dict(n=-1),
                dict(n_frames=0), dict(height=0), dict(width=0), dict(margin_x=-1), dict(margin_y=-1),
                dict(delta=-1.0), dict(delta=float("nan")), dict(stats=None)]


def test_einval_before_any_launch():
    lib = _lib.load()
    assert lib.scflow_scene_visibility(None, None) == -1
    for kw in EINVAL_CASES:
        assert lib.scflow_scene_visibility(ctypes.byref(_args(**kw)), None) == -1, kw
    assert lib.scflow_scene_visibility(ctypes.byref(_args(n=0)), None) == 0          # a no-op
    assert lib.scflow_scene_visibility(ctypes.byref(_args(n_frames=70000)), None) == -2
    assert lib.scflow_scene_visibility(ctypes.byref(_args(width=1 << 25)), None) == -2


def test_scene_args_layout_matches_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f for f, _ in _lib.SceneArgs._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scflow_hip.h"\nint main(){\n'
                    'printf("%zu\\n", sizeof(scflow_scene_args));\n' +
                    "".join(f'printf("%zu\\n", offsetof(scflow_scene_args, {f}));\n' for f in fields) +
                    "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(_lib.SceneArgs)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_lib.SceneArgs, f).offset == off, f
