"""Test-side helper (not a test): the seeded scenes, the closed forms and the comparison rule that
the scene-visibility tests share (``tests/test_scene_host.py``, ``tests/test_gpu_scene.py``).
numpy + ``tests/scene_restatement.py``; the meshes are ``tests/render_cases.py``'s.

Classes: 0 box, 1 tetra, 2 octa, 3 torus(34, 12, 24, 12) (576 faces: three binning passes of 256),
4 an 8×12 ellipsoid with one zero-area face appended, 5 no mesh, 6 a small box.

Cases (``case(name)``; frame_index sorted, K differing per frame, fx ≈ 260 scaled to the frame,
objects at 380–520 mm):

* ``tiny``      5×7, one frame, n = 1, margin (5, 3);
* ``wide``      33×65, two frames of 3 instances, margin (0, 0), no sensor depth;
* ``tall``      65×33, three frames of 1 / 0 / 5 instances, sensor depth (an occluder nearer than
                the objects over one part, zeros over another), pixel_offset 0.5, margin (16, 16),
                delta 0;
* ``crowd``     48×64, n = 70 over three frames of 40 / 24 / 6 instances (40: more than one LDS
                pass of planes, and the two-sweep path without a sensor depth);
* ``crowd_dt``  the same with a sensor depth (one sweep, two passes);
* ``special``   48×64, three frames: six placed instances in frame 0 (wholly outside, across the
                left and top borders, part of its faces at Z ≤ 0, the same class twice, an exact
                duplicate pose), none in frame 1, three in frame 2, one label outside the table, one
                label without a mesh and, last, one frame_index outside the frames; sensor depth;
                margin (5, 3);
* ``special_nodt``  the same without sensor depth, delta 0, pixel_offset 0.5.
"""
from functools import lru_cache

import numpy as np

from tests import render_cases as rc
from tests import scene_restatement as sr

EPS_Z = rc.EPS_Z
CASES = ("tiny", "wide", "tall", "crowd", "crowd_dt", "special", "special_nodt")


@lru_cache(maxsize=None)
def meshes():
    v, f, _ = rc._ell((50, 38, 30), 8, 12)
    f = np.concatenate([np.asarray(f, np.int64), [[0, 5, 5]]])   # a zero-area face
    out = {0: rc.box(45, 35, 25)[:2], 1: rc.tetra()[:2], 2: rc.octa()[:2],
           3: rc.torus(34, 12, 24, 12)[:2], 4: (np.asarray(v, np.float32), f), 6: rc.box(20, 16, 12)[:2]}
    out = {l: (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64)) for l, (v, f) in out.items()}
    for m in out.values():
        for a in m:
            a.setflags(write=False)
    return out


NUM_CLASSES = 7


def _K(H, W, k):
    s = max(H, W) / 64.0
    return np.array([[260.0 * s * (1 + 0.03 * k), 0, W / 2 - 0.3 + 0.4 * k],
                     [0, 255.0 * s * (1 - 0.02 * k), H / 2 + 0.2 - 0.3 * k], [0, 0, 1]], np.float32)


def _place(rng, labels, spread):
    n = len(labels)
    R = np.stack([rc.rotation(int(rng.integers(1 << 30))) for _ in range(n)]).astype(np.float32)
    t = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n),
                  rng.uniform(380, 520, n)], 1).astype(np.float32)
    return R, t


def _sensor(rng, F, H, W):
    d = np.full((F, H, W), 2000.0, np.float32)
    d[:, : H // 3, : W // 2] = 250.0          # an occluder nearer than every object
    d[:, H // 2:, W // 2:] = 0.0              # no measurement
    d[:, H // 3: H // 2] += rng.uniform(0, 50, (F, H // 2 - H // 3, W)).astype(np.float32)
    return d


@lru_cache(maxsize=None)
def case(name):
    """dict(H, W, F, labels, frame_index, R, t, K, depth_test, delta, margin, pixel_offset)."""
    rng = np.random.default_rng({"tiny": 1, "wide": 2, "tall": 3, "crowd": 4, "crowd_dt": 4,
                                 "special": 5, "special_nodt": 5}[name])
    small = (0, 1, 2, 6)
    if name == "tiny":
        H, W, per = 5, 7, [[6]]
        spread, opt = 10, dict(margin=(5, 3))
    elif name == "wide":
        H, W, per = 33, 65, [[3, 0, 4], [1, 3, 2]]
        spread, opt = 45, {}
    elif name == "tall":
        H, W, per = 65, 33, [[4], [], [0, 1, 2, 3, 3]]
        spread, opt = 35, dict(margin=(16, 16), delta=0.0, pixel_offset=0.5, sensor=True)
    elif name in ("crowd", "crowd_dt"):
        H, W = 48, 64
        per = [[small[int(k)] for k in rng.integers(0, 4, c)] for c in (40, 24, 6)]
        spread, opt = 55, dict(sensor=name == "crowd_dt")
    else:
        H, W, per = 48, 64, [[0, 4, 0, 2, 3, 3], [], [1, 4, 6, 9, 5]]
        spread = 40
        opt = dict(margin=(5, 3), sensor=True) if name == "special" else dict(delta=0.0, pixel_offset=0.5)
    F = len(per)
    labels = np.array([l for p in per for l in p], np.int32)
    fidx = np.array([f for f, p in enumerate(per) for _ in p], np.int32)
    R, t = _place(rng, labels, spread)
    if name.startswith("special"):
        t[0] = (900, 0, 450)                   # wholly outside the frame
        t[1] = (-54, -41, 440)                 # across the left and top borders
        t[2] = (5, -4, 20)                     # a box with part of its vertices at Z ≤ 0
        R[5], t[5] = R[4], t[4]                # an exact duplicate pose: the tie goes to index 4
        labels = np.append(labels, 3).astype(np.int32)
        fidx = np.append(fidx, 7).astype(np.int32)   # outside the frames (kept non-decreasing)
        R = np.concatenate([R, R[:1]])
        t = np.concatenate([t, t[:1]])
    K = np.stack([_K(H, W, k) for k in range(F)])
    out = dict(H=H, W=W, F=F, labels=labels, frame_index=fidx, R=R, t=t, K=K,
               depth_test=_sensor(rng, F, H, W) if opt.get("sensor") else None,
               delta=opt.get("delta", 15.0), margin=opt.get("margin", (0, 0)),
               pixel_offset=opt.get("pixel_offset", 0.0))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def restate(c, dtype=np.float64):
    return sr.scene_visibility(meshes(), c["labels"], c["frame_index"], c["R"], c["t"], c["K"], c["H"],
                               c["W"], c["depth_test"], c["delta"], c["margin"], c["pixel_offset"], dtype)


@lru_cache(maxsize=None)
def reference(name, fp32=False):
    """The restatement of a case (float64, or the float32 stand-in), shared and read-only."""
    return restate(case(name), np.float32 if fp32 else np.float64)


# ------------------------------------------------------------------------------ closed forms
def _square(x0, x1, y0, y1, z, f=100.0):
    """A fronto-parallel two-triangle square at depth z whose edges project to x0, x1, y0, y1
    (cx = cy = 0, fx = fy = f, R = 1, t = (0, 0, z))."""
    X0, X1, Y0, Y1 = (c * z / f for c in (x0, x1, y0, y1))
    v = np.array([[X0, Y0, 0], [X1, Y0, 0], [X1, Y1, 0], [X0, Y1, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int64)


def closed_forms():
    """[(name, meshes, call arguments, {instance: {stat: value}})]: a 64×48 frame, squares with
    edges on half-integer coordinates.  No sample is on an outer edge, and the sides (10 × 7 and
    5 × 10) are chosen so that none is on the diagonal the two triangles share either (a sample on
    an edge has a zero weight and is not covered): the counts are exact."""
    K = np.array([[[100.0, 0, 0], [0, 100.0, 0], [0, 0, 1]]], np.float32)
    eye = np.eye(3, dtype=np.float32)

    def args(zs, **kw):
        n = len(zs)
        return dict(dict(labels=np.arange(n, dtype=np.int32), frame_index=np.zeros(n, np.int32),
                         R=np.stack([eye] * n), t=np.array([[0, 0, z] for z in zs], np.float32), K=K,
                         H=48, W=64, depth_test=None, delta=15.0, margin=(0, 0), pixel_offset=0.0), **kw)
    far = _square(9.5, 19.5, 7.5, 14.5, 500.0)            # covers [10, 20) × [8, 15)
    full = dict(px_count_all=70, px_count_valid=70, px_count_visib=70, bbox_obj=[10, 8, 10, 7],
                bbox_visib=[10, 8, 10, 7], visib_fract=1.0)
    half = dict(full, px_count_visib=35, bbox_visib=[15, 8, 5, 7], visib_fract=0.5)
    near5 = dict(px_count_all=50, px_count_visib=50, bbox_obj=[10, 6, 5, 10], visib_fract=1.0)
    left = _square(-6.5, 3.5, 7.5, 14.5, 500.0)           # covers [−6, 4) × [8, 15)
    sensor = lambda v: np.full((1, 48, 64), v, np.float32)  # noqa: E731
    return [
        ("alone", {0: far}, args([500.0]), {0: full}),
        ("half_hidden", {0: far, 1: _square(9.5, 14.5, 5.5, 15.5, 400.0)}, args([500.0, 400.0]),
         {0: half, 1: near5}),
        ("gap_10mm", {0: far, 1: _square(9.5, 14.5, 5.5, 15.5, 490.0)}, args([500.0, 490.0]),
         {0: full, 1: near5}),
        ("gap_10mm_delta_0", {0: far, 1: _square(9.5, 14.5, 5.5, 15.5, 490.0)},
         args([500.0, 490.0], delta=0.0), {0: half, 1: near5}),
        ("left_border", {0: left}, args([500.0]),
         {0: dict(px_count_all=28, px_count_visib=28, bbox_obj=[0, 8, 4, 7], bbox_visib=[0, 8, 4, 7])}),
        ("left_border_margin", {0: left}, args([500.0], margin=(5, 2)),
         {0: dict(px_count_all=63, px_count_valid=28, px_count_visib=28, bbox_obj=[-5, 8, 9, 7],
                  bbox_visib=[0, 8, 4, 7], visib_fract=28 / 63)}),
        ("sensor_nearer", {0: far}, args([500.0], depth_test=sensor(300.0)),
         {0: dict(full, px_count_visib=0, bbox_visib=[-1, -1, -1, -1], visib_fract=0.0)}),
        ("sensor_zeros", {0: far}, args([500.0], depth_test=sensor(0.0)), {0: dict(full, px_count_valid=0)}),
    ]


def stats_dict(row):
    s = [int(v) for v in row]
    return dict(px_count_all=s[0], px_count_valid=s[1], px_count_visib=s[2], bbox_obj=s[3:7],
                bbox_visib=s[7:11], visib_fract=s[2] / s[0] if s[0] else 0.0)


# ------------------------------------------------------------------------------ the rule
def _edges(mask, ox=0, oy=0):
    rr, cc = np.nonzero(mask)
    if len(rr) == 0:
        return None
    return (int(cc.min()) - ox, int(rr.min()) - oy, int(cc.max()) - ox, int(rr.max()) - oy)


def _box_ok(got, sure, maybe):
    """``got`` (x, y, w, h) against the box edges of the surely-set pixels and of those plus the
    ambiguous ones: every edge between the two, hence exact where they agree."""
    lo, hi = _edges(sure[0], *sure[1:]), _edges(maybe[0], *maybe[1:])
    if tuple(got) == (-1, -1, -1, -1):
        return lo is None
    if hi is None:
        return False
    g = (got[0], got[1], got[0] + got[2] - 1, got[1] + got[3] - 1)
    if lo is None:
        return hi[0] <= g[0] and hi[1] <= g[1] and g[2] <= hi[2] and g[3] <= hi[3]
    return hi[0] <= g[0] <= lo[0] and hi[1] <= g[1] <= lo[1] and lo[2] <= g[2] <= hi[2] and lo[3] <= g[3] <= hi[3]


def compare(got, ref, c):
    """The GPU tests' rule (also applied to the float32 stand-in on the CPU).  ``got``: dict of numpy
    outputs; ``ref``: the float64 restatement; ``c``: the case.  Asserts it and returns the figures."""
    fidx, F, (mx, my), H, W = c["frame_index"], c["F"], c["margin"], c["H"], c["W"]
    amb_f, amb_c = sr.ambiguous(ref, np.clip(fidx, 0, F - 1), F, c["margin"])
    fig = dict(ambiguous=int(amb_f.sum()), dz=0.0, dstat=0, flips=0)
    ok = ~amb_f
    fig["flips"] += int((got["inst_id"] != ref["inst_id"]).sum())
    assert np.array_equal(got["inst_id"][ok], ref["inst_id"][ok]), "inst_id"
    for name in ("depth_scene",):
        both = (got[name] > 0) & (ref[name] > 0)
        assert np.array_equal((got[name] > 0)[ok], (ref[name] > 0)[ok]), name
        if both.any():
            fig["dz"] = max(fig["dz"], float((np.abs(got[name][both] - ref[name][both]) / ref[name][both]).max()))
    for i in range(len(fidx)):
        f = int(fidx[i])
        if ref["skipped"][i]:
            assert not got["depth_inst"][i].any() and not got["mask_visib"][i].any(), i
            assert got["stats"][i].tolist() == [0, 0, 0] + [-1] * 8 + [0], i
            continue
        o, oc = ok[f], ~amb_c[f]
        gd, rd = got["depth_inst"][i], ref["depth_inst"][i]
        fig["flips"] += int(((gd > 0) != (rd > 0)).sum()) + int((got["mask_visib"][i] != ref["mask_visib"][i]).sum())
        assert np.array_equal((gd > 0)[o], (rd > 0)[o]), ("depth_inst > 0", i)
        assert np.array_equal(got["mask_visib"][i][o], ref["mask_visib"][i][o]), ("mask_visib", i)
        both = (gd > 0) & (rd > 0)
        if both.any():
            fig["dz"] = max(fig["dz"], float((np.abs(gd[both] - rd[both]) / rd[both]).max()))
        # counters: within the ambiguous pixels of the instance's footprint
        foot_c = ref["cover_canvas"][i] | (ref["edge_margin"][i] < ref["edge_thr"][i])
        foot_f = foot_c[my:my + H, mx:mx + W]
        slack_c, slack_f = int((foot_c & amb_c[f]).sum()), int((foot_f & amb_f[f]).sum())
        gs, rs = got["stats"][i], ref["stats"][i]
        d = [abs(int(gs[k]) - int(rs[k])) for k in range(3)]
        fig["dstat"] = max(fig["dstat"], *d)
        assert d[0] <= slack_c and d[1] <= slack_f and d[2] <= slack_f, ("counters", i, d, slack_c, slack_f)
        assert gs[11] == 0
        # boxes: exact where the ambiguous pixels cannot touch the edge
        cov_c, vis = ref["cover_canvas"][i], ref["mask_visib"][i] > 0
        assert _box_ok(gs[3:7], (cov_c & oc, mx, my), (cov_c | (foot_c & amb_c[f]), mx, my)), ("bbox_obj", i)
        assert _box_ok(gs[7:11], (vis & o, 0, 0), (vis | (foot_f & amb_f[f]), 0, 0)), ("bbox_visib", i)
    assert fig["dz"] <= EPS_Z, fig["dz"]
    return fig
