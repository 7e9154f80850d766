"""Test-side helper (not a test): the seeded inputs that the CPU and GPU tests of the BOP metrics
share (``tests/test_bop_metrics_host.py``, ``tests/test_gpu_bop_metrics.py``), and their
restatement results, computed once per process (``tests/bop_restatement.py``).  numpy only.

Every array is rounded to float32 before anything reads it: the restatement evaluates in float64
the very numbers the kernels get.
"""
from functools import lru_cache

import numpy as np

from tests import bop_restatement as br

MAX_POINTS = 1000
WIDTH = 640
CAM_K = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])

# ------------------------------------------------------------------------------ MSSD / MSPD
_DISC = [-1.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0, -2.0, 0.0, 0.0, 1.0, 0.5, 0.0, 0.0, 0.0, 1.0]  # 180° about z
_CONT = {"axis": [0.0, 0.0, 1.0], "offset": [3.0, -2.0, 5.0]}
SYM_KINDS = {1: {}, 2: {"symmetries_discrete": [_DISC]}, 315: {"symmetries_continuous": [_CONT]},
             630: {"symmetries_discrete": [_DISC], "symmetries_continuous": [_CONT]}}
POINT_COUNTS = (1, 63, 65, 1000)


@lru_cache(maxsize=None)
def classes():
    """17 classes: every P ∈ {1, 63, 65, 1000} with every S ∈ {1, 2, 315, 630}, and a last class
    with no vertex.  → (points [17, 1000, 3] float32 with NaN padding, counts [17] int32,
    models_info {obj_id str: entry} with diameters, [(P, S)] per class)."""
    rng = np.random.default_rng(2019)
    kinds = [(p, s) for p in POINT_COUNTS for s in SYM_KINDS] + [(0, 1)]
    points = np.full((len(kinds), MAX_POINTS, 3), np.nan, np.float32)
    counts = np.zeros(len(kinds), np.int32)
    info = {}
    for c, (p, s) in enumerate(kinds):
        points[c, :p] = rng.uniform(-80.0, 80.0, (p, 3)).astype(np.float32)
        counts[c] = p
        info[str(c + 1)] = dict(SYM_KINDS[s], diameter=100.0 + 5.0 * c)
    points.setflags(write=False)
    counts.setflags(write=False)
    return points, counts, info, kinds


def _small_rotation(rng, max_angle):
    axis = rng.normal(size=3)
    return br.rot_axis_angle(axis, rng.uniform(0.0, max_angle))


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


@lru_cache(maxsize=None)
def pose_batch(n, seed=0):
    """n (estimate, GT) pairs over ``classes()``: labels cycle through the classes (n = 1: the
    P = 1000, S = 630 class); t_z ∈ [500, 1500], estimates within 0.3 rad and 20 mm of the GT."""
    rng = np.random.default_rng(100 + seed)
    _, _, _, kinds = classes()
    labels = np.arange(n) % len(kinds) if n > 1 else np.array([kinds.index((1000, 630))])
    Rg = np.stack([_random_rotation(rng) for _ in range(n)])
    tg = np.stack([np.array([rng.uniform(-150, 150), rng.uniform(-150, 150), rng.uniform(500, 1500)])
                   for _ in range(n)])
    Re = np.stack([Rg[i] @ _small_rotation(rng, 0.3) for i in range(n)])
    te = tg + rng.uniform(-20.0, 20.0, (n, 3))
    K = np.repeat(CAM_K[None], n, 0)
    out = dict(labels=labels.astype(np.int64), R_est=Re.astype(np.float32), t_est=te.astype(np.float32),
               R_gt=Rg.astype(np.float32), t_gt=tg.astype(np.float32), K=K.astype(np.float32))
    for a in out.values():
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def pose_reference(n, seed=0):
    """(mssd [n], mspd [n], mssd bound, mspd bound) of ``pose_batch`` by the restatement.  The
    bounds are fp32 ulps at the batch's magnitudes: MSSD 32·2⁻²³·(max |t| + max ‖x‖), MSPD
    64·2⁻²³·max(|u|, |v|, W)."""
    points, counts, info, _ = classes()
    b = pose_batch(n, seed)
    sets = {c: br.symmetry_set(info[str(c + 1)]) for c in set(b["labels"].tolist())}
    s, p, big_uv, big_x = [], [], float(WIDTH), 0.0
    for i, lab in enumerate(b["labels"]):
        v = points[lab, :counts[lab]].astype(np.float64)
        a = (b["R_est"][i], b["t_est"][i], b["R_gt"][i], b["t_gt"][i])
        s.append(br.mssd(*a, v, sets[lab]))
        p.append(br.mspd(*a, b["K"][i], v, sets[lab]))
        if len(v):
            big_x = max(big_x, float(np.linalg.norm(v, axis=1).max()))
            for R, t in ((a[0], a[1]), (a[2], a[3])):
                h = (v @ R.astype(np.float64).T + t) @ b["K"][i].astype(np.float64).T
                big_uv = max(big_uv, float(np.abs(h[:, :2] / h[:, 2:3]).max()))
    big_t = float(max(np.abs(b["t_est"]).max(), np.abs(b["t_gt"]).max()))
    return (np.array(s), np.array(p), 32.0 * 2.0 ** -23 * (big_t + big_x), 64.0 * 2.0 ** -23 * big_uv)


# ------------------------------------------------------------------------------ VSD
VSD_SHAPES = ((5, 7), (33, 65), (48, 64), (64, 64))
VSD_NS = (1, 6, 70)
VSD_TAUS = {1: (0.2,), 10: tuple(round(0.05 * k, 2) for k in range(1, 11)),
            16: tuple(round(0.03 * k, 2) for k in range(1, 17))}
DELTA = 15.0


def vsd_case_list():
    """The 24 cases: every shape × N × (diameter given or not); n_taus and the objects per frame
    (2 or 3) cycle with the case number."""
    out = []
    for h, w in VSD_SHAPES:
        for n in VSD_NS:
            for normalised in (False, True):
                i = len(out)
                out.append((h, w, n, (1, 10, 16)[i % 3], normalised, 2 + (i // 3) % 2))
    return out


@lru_cache(maxsize=None)
def vsd_case(h, w, n, n_taus, normalised, per_frame, seed=0):
    """Disc-shaped tilted depth blobs at 700 to 900 mm for the GT, the estimate displaced by up to
    3 px and ±40 mm, test depth uniform ±60 mm around them with 15 % zeros."""
    rng = np.random.default_rng([seed, h, w, n, n_taus, int(normalised)])
    n_frames = (n + per_frame - 1) // per_frame
    frame_index = (np.arange(n) // per_frame).astype(np.int32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    est, gt = np.zeros((n, h, w)), np.zeros((n, h, w))
    test_base = np.full((n_frames, h, w), 800.0)
    for i in range(n):
        cx0, cy0 = rng.uniform(0.2 * w, 0.8 * w), rng.uniform(0.2 * h, 0.8 * h)
        rad = rng.uniform(0.25, 0.45) * min(h, w) + 1.0
        base, sx, sy = rng.uniform(700.0, 900.0), rng.uniform(-2.0, 2.0), rng.uniform(-2.0, 2.0)
        plane = base + sx * (xx - cx0) + sy * (yy - cy0)
        m = (xx - cx0) ** 2 + (yy - cy0) ** 2 <= rad * rad
        gt[i] = np.where(m, plane, 0.0)
        dx, dy, dz = rng.uniform(-3.0, 3.0), rng.uniform(-3.0, 3.0), rng.uniform(-40.0, 40.0)
        me = (xx - cx0 - dx) ** 2 + (yy - cy0 - dy) ** 2 <= rad * rad
        est[i] = np.where(me, plane + dz, 0.0)
        f = frame_index[i]
        test_base[f] = np.where(m, plane, test_base[f])
    test = test_base + rng.uniform(-60.0, 60.0, test_base.shape)
    test[rng.uniform(size=test.shape) < 0.15] = 0.0
    K = np.repeat(np.array([[1.2 * w, 0, 0.5 * w - 0.3], [0, 1.25 * w, 0.5 * h + 0.2], [0, 0, 1.0]])[None], n, 0)
    diam = rng.uniform(100.0, 200.0, n)
    out = dict(depth_est=est.astype(np.float32), depth_gt=gt.astype(np.float32),
               depth_test=test.astype(np.float32), frame_index=frame_index, K=K.astype(np.float32),
               diameter=diam.astype(np.float32) if normalised else None,
               # without a diameter the tolerances are in mm: the same fractions of 100 mm
               taus=VSD_TAUS[n_taus] if normalised else tuple(100.0 * t for t in VSD_TAUS[n_taus]))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def vsd_reference(*case):
    """(counts [n, 2 + n_taus] int64, ambiguous pixels of the case) by the restatement."""
    c = vsd_case(*case)
    taus = np.asarray(c["taus"], np.float32).astype(np.float64)
    counts, amb = [], 0
    for i in range(c["depth_est"].shape[0]):
        d = None if c["diameter"] is None else float(c["diameter"][i])
        k, a, _ = br.vsd_counts(c["depth_est"][i], c["depth_gt"][i], c["depth_test"][c["frame_index"][i]],
                                c["K"][i], DELTA, taus, d)
        counts.append(k)
        amb += a
    return np.stack(counts), amb


# ------------------------------------------------------------------------------ average recall
AR_SIZE = 64  # renders and frames of the end-to-end case
# perturbation of estimate i: (rotation about the object's x axis in rad, translation in mm)
AR_PERTURBATIONS = ((0.0, (0.3, 0.0, 0.0)), (0.02, (1.0, -1.0, -3.0)), (0.05, (2.0, 2.0, -8.0)),
                    (0.08, (-4.0, 5.0, -6.0)), (0.18, (12.0, -9.0, 25.0)), (0.30, (22.0, 16.0, -45.0)),
                    (0.45, (-38.0, 30.0, 70.0)), (0.80, (70.0, -55.0, 140.0)))


@lru_cache(maxsize=None)
def ar_case():
    """Eight ellipsoids (label i = object i, ``tests/render_cases.py``'s mesh builder) seen in a
    64² frame each, with the perturbations above; diameters = twice the largest semi-axis."""
    from tests import render_cases as rc
    rng = np.random.default_rng(77)
    meshes, diam = {}, []
    for i in range(8):
        semi = (40.0 + 3.0 * i, 30.0 + 2.0 * i, 24.0 + i)
        meshes[i] = rc._ell(semi, 8, 12)
        diam.append(2.0 * semi[0])
    Rg = np.stack([_random_rotation(rng) for _ in range(8)])
    tg = np.stack([np.array([rng.uniform(-8, 8), rng.uniform(-8, 8), rng.uniform(650, 800)]) for _ in range(8)])
    Re = np.stack([Rg[i] @ br.rot_axis_angle([1.0, 0.0, 0.0], AR_PERTURBATIONS[i][0]) for i in range(8)])
    te = tg + np.array([p[1] for p in AR_PERTURBATIONS])
    K = np.repeat(np.array([[260.0, 0, 31.5], [0, 260.0, 31.5], [0, 0, 1.0]])[None], 8, 0)
    out = dict(meshes=meshes, diameters=np.array(diam), labels=np.arange(8, dtype=np.int64),
               R_est=Re.astype(np.float32), t_est=te.astype(np.float32), R_gt=Rg.astype(np.float32),
               t_gt=tg.astype(np.float32), K=K.astype(np.float32))
    return out


AR_DEPTH_SEED = 11


def ar_test_depth(z_gt, seed=AR_DEPTH_SEED):
    """The end-to-end case's sensor depth from the GT renders' zbuf [8, S, S]: the GT depth ± 25 mm
    where the object is, nothing elsewhere, 10 % dropped."""
    rng = np.random.default_rng(seed)
    z_gt = np.asarray(z_gt)
    test = np.where(z_gt > 0, z_gt + rng.uniform(-25.0, 25.0, z_gt.shape), 0.0)
    test[rng.uniform(size=test.shape) < 0.1] = 0.0
    return test.astype(np.float32)


def ar_vsd_reference(z_est, z_gt, test, rows=AR_SIZE):
    """(counts [8, 12], ambiguous pixels [8]) of the end-to-end case by the restatement, on given
    depth renders (the renderer's own zbuf on the GPU, the CPU oracle's in the host test)."""
    c = ar_case()
    taus = np.asarray([round(0.05 * k, 2) for k in range(1, 11)], np.float32).astype(np.float64)
    out = [br.vsd_counts(z_est[i, :rows], z_gt[i, :rows], test[i, :rows], c["K"][i], DELTA, taus,
                         float(np.float32(c["diameters"][i]))) for i in range(8)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def vsd_threshold_margins(counts):
    """Per object, the smallest |e_k − θ| over the BOP19 τ and θ."""
    e = br.vsd_errors(counts)
    th = np.array([round(0.05 * k, 2) for k in range(1, 11)])
    return np.abs(e[:, :, None] - th[None, None, :]).min((1, 2))


@lru_cache(maxsize=None)
def ar_reference():
    """(mssd [8], mspd [8]) of ``ar_case`` by the restatement (no symmetries)."""
    c = ar_case()
    ident = [(np.eye(3), np.zeros(3))]
    s, p = [], []
    for i in range(8):
        v = np.asarray(c["meshes"][i][0], np.float64)
        a = (c["R_est"][i], c["t_est"][i], c["R_gt"][i], c["t_gt"][i])
        s.append(br.mssd(*a, v, ident))
        p.append(br.mspd(*a, c["K"][i], v, ident))
    return np.array(s), np.array(p)


def threshold_margins(errors, thresholds):
    """Smallest |error − threshold| over all pairs; thresholds [T] or [M, T]."""
    e = np.asarray(errors, np.float64)
    th = np.asarray(thresholds, np.float64)
    th = th[None] if th.ndim == 1 else th
    return float(np.abs(e[:, None] - th).min())
