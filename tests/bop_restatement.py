"""Test-side helper (not a test): a plain numpy float64 restatement of the BOP19 pose errors, written
from their definitions (bop_toolkit's pose_error.py / misc.py restated there, the
toolkit itself is absent) with per-symmetry and per-pixel loops.  It shares no code with
``scflow_amd.bop_metrics`` or the HIP kernels; the CPU and GPU tests of the BOP metrics share it.

``vsd_counts`` also reports the *ambiguous* pixels of a case: those where some decision of the
definition (the two ``M − T ≤ δ`` tests, each ``≥ τ_k`` test) has a margin below ε = 64·2⁻²³·(the
largest distance in the case) mm (ε / d for the normalised cost): an fp32 evaluation may decide
them either way, so a count may differ from this restatement's by at most their number.
"""
import math

import numpy as np


# ------------------------------------------------------------------------------ symmetry sets
def rot_axis_angle(axis, angle):
    """cos·I + sin·[a]× + (1 − cos)·a aᵀ."""
    a = np.asarray(axis, np.float64)
    a = a / math.sqrt(float(a @ a))
    c, s = math.cos(angle), math.sin(angle)
    cross = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], np.float64)
    return c * np.eye(3) + s * cross + (1 - c) * np.outer(a, a)


def symmetry_set(info, step=0.01):
    """List of (R [3,3], t [3]) of a models_info entry (None / {}: the identity alone)."""
    info = info or {}
    disc = [(np.eye(3), np.zeros(3))]
    for s in info.get("symmetries_discrete", []):
        m = np.array(s, np.float64).reshape(4, 4)
        disc.append((m[:3, :3], m[:3, 3]))
    cont = []
    for c in info.get("symmetries_continuous", []):
        count = int(np.ceil(np.pi / step))
        off = np.array(c["offset"], np.float64)
        for i in range(count):
            R = rot_axis_angle(c["axis"], 2.0 * np.pi * i / count)
            cont.append((R, off - R @ off))
    if not cont:
        return disc
    return [(Rc @ Rd, Rc @ td + tc) for Rc, tc in cont for Rd, td in disc]


# ------------------------------------------------------------------------------ MSSD / MSPD
def _proj(K, X):
    h = X @ np.asarray(K, np.float64).T
    return h[:, :2] / h[:, 2:3]


def mssd(R_e, t_e, R_g, t_g, verts, syms):
    verts = np.asarray(verts, np.float64)
    if len(verts) == 0:
        return np.inf
    pe = verts @ np.asarray(R_e, np.float64).T + np.asarray(t_e, np.float64)
    best = np.inf
    for Rs, ts in syms:
        pg = (verts @ Rs.T + ts) @ np.asarray(R_g, np.float64).T + np.asarray(t_g, np.float64)
        best = min(best, float(np.sqrt(((pe - pg) ** 2).sum(1)).max()))
    return best


def mspd(R_e, t_e, R_g, t_g, K, verts, syms):
    verts = np.asarray(verts, np.float64)
    if len(verts) == 0:
        return np.inf
    ue = _proj(K, verts @ np.asarray(R_e, np.float64).T + np.asarray(t_e, np.float64))
    best = np.inf
    for Rs, ts in syms:
        ug = _proj(K, (verts @ Rs.T + ts) @ np.asarray(R_g, np.float64).T + np.asarray(t_g, np.float64))
        best = min(best, float(np.sqrt(((ue - ug) ** 2).sum(1)).max()))
    return best


# ------------------------------------------------------------------------------ VSD
def _dist(D, x, y, K):
    X = (x - K[0][2]) * D / K[0][0]
    Y = (y - K[1][2]) * D / K[1][1]
    return math.sqrt(X * X + Y * Y + D * D)


def vsd_counts(D_est, D_gt, D_test, K, delta, taus, diameter=None):
    """(counts [2 + n_taus] = (|U|, |I|, cost_k …), ambiguous pixels, largest distance) of one
    pair, pixel by pixel.  Depth maps [H, W]; ``diameter`` None: the cost is not normalised."""
    D_est, D_gt, D_test = (np.asarray(a, np.float64) for a in (D_est, D_gt, D_test))
    K = np.asarray(K, np.float64)
    H, W = D_gt.shape
    taus = [float(t) for t in taus]
    # largest distance first: it sets ε
    far = 0.0
    rows = []
    for y in range(H):
        for x in range(W):
            if D_est[y, x] <= 0 and D_gt[y, x] <= 0:
                continue  # neither mask holds the pixel: it enters no count
            me, mg, mt = (_dist(float(D[y, x]), x, y, K) if D[y, x] > 0 else 0.0 for D in (D_est, D_gt, D_test))
            far = max(far, me, mg, mt)
            rows.append((me, mg, mt))
    eps = 64.0 * 2.0 ** -23 * far
    counts = [0] * (2 + len(taus))
    ambiguous = 0
    for me, mg, mt in rows:
        amb = False

        def vis(m):
            nonlocal amb
            if m > 0 and mt != 0 and abs((m - mt) - delta) < eps:
                amb = True
            return ((m - mt <= delta) or (mt == 0)) and (m > 0)
        v_gt = vis(mg)
        v_est = vis(me) or (v_gt and me > 0)
        if v_gt or v_est:
            counts[0] += 1
        if v_gt and v_est:
            counts[1] += 1
        if mg > 0 and me > 0:  # the pixel is, or within ε could be, in the intersection
            r = abs(mg - me)
            e = eps
            if diameter is not None:
                r, e = r / diameter, eps / diameter
            for k, tau in enumerate(taus):
                if abs(r - tau) < e:
                    amb = True
                if v_gt and v_est and r >= tau:
                    counts[2 + k] += 1
        ambiguous += amb
    return np.array(counts, np.int64), ambiguous, far


def vsd_errors(counts):
    """e_k = (cost_k + |U| − |I|) / |U|, 1 where |U| = 0; counts [..., 2 + n_taus]."""
    c = np.asarray(counts, np.float64)
    u, i = c[..., :1], c[..., 1:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(u > 0, (c[..., 2:] + u - i) / u, 1.0)


# ------------------------------------------------------------------------------ recall
def average_recall(vsd_e, mssd_e, mspd_e, diameters, width, targets):
    """BOP19 AR with explicit loops: dict(AR_VSD, AR_MSSD, AR_MSPD, AR)."""
    thetas = [round(0.05 * k, 2) for k in range(1, 11)]
    px = [5.0 * k * width / 640.0 for k in range(1, 11)]
    idx = [i for i, t in enumerate(targets) if t]
    n = len(idx)

    def rec(pred):
        return sum(1 for i in idx if pred(i)) / n if n else 0.0
    n_taus = np.asarray(vsd_e).shape[1]
    r_vsd = [rec(lambda i: vsd_e[i][k] < th) for k in range(n_taus) for th in thetas]
    r_mssd = [rec(lambda i: mssd_e[i] < th * diameters[i]) for th in thetas]
    r_mspd = [rec(lambda i: mspd_e[i] < th) for th in px]
    out = dict(AR_VSD=sum(r_vsd) / len(r_vsd), AR_MSSD=sum(r_mssd) / len(r_mssd),
               AR_MSPD=sum(r_mspd) / len(r_mspd))
    out["AR"] = (out["AR_VSD"] + out["AR_MSSD"] + out["AR_MSPD"]) / 3.0
    out.update(recall_vsd=np.array(r_vsd).reshape(n_taus, len(thetas)), recall_mssd=np.array(r_mssd),
               recall_mspd=np.array(r_mspd))
    return out
