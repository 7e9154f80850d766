"""numpy fp64 restatement of the batched RANSAC-PnP contract (kernels in
scflow_amd/csrc/pnp.hip), written from the contract and not from the kernels: the same counter hash
and sampling, ``np.roots`` for the P3P quartic, SVD absolute orientation, a plain-loop fp64 scorer
and a Gauss-Newton refinement whose per-point part can also be run in ``np.float32``.

Five steps per sample: correspondences (compacted in ascending pixel order) → ``hyps`` P3P
hypotheses on hashed 4-point samples → inlier counts → winner (highest count, lowest index) →
Gauss-Newton on the winner's inlier set.  Helper module, like ``tests/raft_restatement.py``.
"""
import numpy as np

COLLINEAR_SIN2 = 1e-4  # a sample whose object-space triangle has sin² of an angle at P0 below this is invalid


def lowbias32(x):
    """The 32-bit integer hash of the contract (works on python ints and uint32/uint64 arrays)."""
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def sample_indices(b, hyps, count, seed=0):
    """[hyps, 4] int64: s_k = (lowbias32(((b·hyps + h)·4 + k) ^ seed) · count) >> 32."""
    h = np.arange(hyps, dtype=np.uint64)[:, None]
    k = np.arange(4, dtype=np.uint64)[None, :]
    ctr = ((np.uint64(b * hyps) + h) * np.uint64(4) + k) & np.uint64(0xFFFFFFFF)
    r = lowbias32(ctr ^ np.uint64(seed & 0xFFFFFFFF))
    return ((r * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def correspondences(points, flow, valid=None):
    """points [H, W, 4] (X, Y, Z, depth > 0), flow [2, H, W], valid [H, W] or None →
    (corr [count, 5] float32 rows (X, Y, Z, x + flow_x, y + flow_y) in ascending pixel order, the
    pixel indices)."""
    H, W, _ = points.shape
    ok = points[..., 3].reshape(-1) > 0
    if valid is not None:
        ok &= np.asarray(valid).reshape(-1) != 0
    p = np.flatnonzero(ok)
    xs, ys = (p % W).astype(np.float32), (p // W).astype(np.float32)
    f = np.asarray(flow, np.float32).reshape(2, -1)
    corr = np.empty((len(p), 5), np.float32)
    corr[:, :3] = points.reshape(-1, 4)[p, :3]
    corr[:, 3] = xs + f[0, p]
    corr[:, 4] = ys + f[1, p]
    return corr, p


def project(K, R, t, X):
    """→ (uv [n, 2], camera z [n]) in fp64."""
    Xc = X @ R.T + t
    uvw = Xc @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return uvw[:, :2] / uvw[:, 2:3], Xc[:, 2]


def _kabsch(P, Q):
    """Rotation and translation taking the rows of P onto the rows of Q (SVD)."""
    pc, qc = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - qc).T @ (P - pc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, qc - R @ pc


def p3p(X, uv, K):
    """Grunert's P3P on three correspondences → list of (R, t).  With the unit bearings j_i of the
    image points, cosines ca = j1·j2, cb = j0·j2, cg = j0·j1, side lengths a = |X1X2|, b = |X0X2|,
    c = |X0X1| and distances s1 = u·s0, s2 = v·s0, eliminating s0 gives u = N(v)/D(v),
    N = (k − 1)v² − 2k·cb·v + 1 + k, D = 2(cg − v·ca), k = (a² − c²)/b², and the quartic
    N² + D²·(1 − q(1 + v² − 2v·cb)) − 2cg·N·D = 0, q = c²/b² (Haralick et al. 1994, eqs. of Grunert)."""
    X = np.asarray(X, np.float64)
    d1, d2 = X[1] - X[0], X[2] - X[0]
    cr = np.cross(d1, d2)
    if not cr @ cr > COLLINEAR_SIN2 * (d1 @ d1) * (d2 @ d2):
        return []
    Kinv = np.linalg.inv(K)
    j = np.concatenate([uv, np.ones((3, 1))], 1) @ Kinv.T
    j /= np.linalg.norm(j, axis=1, keepdims=True)
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    a2, b2, c2 = (X[1] - X[2]) @ (X[1] - X[2]), d2 @ d2, d1 @ d1
    k, q = (a2 - c2) / b2, c2 / b2
    N = np.array([k - 1.0, -2.0 * k * cb, 1.0 + k])
    D = np.array([-2.0 * ca, 2.0 * cg])
    Wq = np.array([-q, 2.0 * q * cb, 1.0 - q])
    poly = np.polymul(N, N) + np.polymul(np.polymul(D, D), Wq)
    poly[1:] -= 2.0 * cg * np.polymul(N, D)
    if not np.all(np.isfinite(poly)) or poly[0] == 0.0:
        return []
    out = []
    for v in np.roots(poly):
        if abs(v.imag) > 1e-9 * max(1.0, abs(v.real)) or not v.real > 0:
            continue
        v = v.real
        den = np.polyval(D, v)
        if den == 0.0:
            continue
        u = np.polyval(N, v) / den
        s0sq = b2 / (1.0 + v * v - 2.0 * v * cb)
        if not (u > 0 and s0sq > 0 and np.isfinite(u) and np.isfinite(s0sq)):
            continue
        s0 = np.sqrt(s0sq)
        Q = j * np.array([s0, u * s0, v * s0])[:, None]
        R, t = _kabsch(X, Q)
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
            out.append((R, t))
    return out


def hypotheses(corr, K, b, hyps, seed=0):
    """→ dict(idx [hyps, 4], valid [hyps] bool, R [hyps, 3, 3], t [hyps, 3], P [hyps, 3, 4] = K·[R|t])."""
    K = np.asarray(K, np.float64)
    count = len(corr)
    idx = sample_indices(b, hyps, count, seed)
    valid = np.zeros(hyps, bool)
    Rs, ts = np.tile(np.eye(3), (hyps, 1, 1)), np.zeros((hyps, 3))
    c64 = corr.astype(np.float64)
    for h in range(hyps):
        s = idx[h]
        if count < 4 or len(set(s.tolist())) < 4:
            continue
        best = None
        for R, t in p3p(c64[s[:3], :3], c64[s[:3], 3:], K):
            uv, z = project(K, R, t, c64[s[3:], :3])
            e = np.linalg.norm(uv[0] - c64[s[3], 3:])
            if np.isfinite(e) and z[0] > 0 and (best is None or e < best[0]):
                best = (e, R, t)
        if best is not None:
            valid[h], Rs[h], ts[h] = True, best[1], best[2]
    P = K @ np.concatenate([Rs, ts[:, :, None]], 2)
    return dict(idx=idx, valid=valid, R=Rs, t=ts, P=P)


def reproj_errors(corr, P):
    """fp64 reprojection error [n] (inf where the camera-frame z ≤ 0) of every correspondence under
    one 3×4 projection P = K·[R|t]."""
    c = corr.astype(np.float64)
    x = c[:, :3] @ P[:, :3].T + P[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.hypot(x[:, 0] / x[:, 2] - c[:, 3], x[:, 1] / x[:, 2] - c[:, 4])
    return np.where(x[:, 2] > 0, e, np.inf)


def score(corr, P, valid, thr=3.0):
    """→ (score [hyps] int, band [hyps] int: points whose fp64 error lies within 1e-2 px of thr)."""
    s, band = np.zeros(len(P), np.int64), np.zeros(len(P), np.int64)
    for h in range(len(P)):
        if valid[h]:
            e = reproj_errors(corr, np.asarray(P[h], np.float64))
            s[h] = int((e < thr).sum())
            band[h] = int((np.abs(e - thr) <= 1e-2).sum())
    return s, band


def winner(scores):
    """Highest score, lowest index on ties."""
    return int(np.argmax(scores))


def _exp_so3(w):
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * (Wx @ Wx)


def refine(corr, inliers, R, t, K, iters=10, per_point=np.float64):
    """Gauss-Newton on the fixed inlier set with the left perturbation R ← exp(ω)R, t ← exp(ω)t + τ.
    Residuals and Jacobians per point in ``per_point`` (fp64 as the kernel computes them, or fp32:
    the run whose distance from the fp64 run is the tests' tolerance unit d); the 6×6 normal
    equations are accumulated and solved (Cholesky) in fp64.  A failed factorisation stops
    and keeps the last pose.  K is upper triangular with K[2, 2] = 1."""
    R, t = np.asarray(R, np.float64).copy(), np.asarray(t, np.float64).copy()
    # a start rounded to fp32 is not orthonormal, and exp(ω)·R keeps the defect: nearest rotation first
    U, _, Vt = np.linalg.svd(R)
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    c = corr[np.asarray(inliers, bool)].astype(per_point)
    Kp = np.asarray(K, np.float64).astype(per_point)
    X, Y, Z = c[:, 0], c[:, 1], c[:, 2]
    for _ in range(iters):
        # elementwise, each operation rounded on its own in the stated (left to right) order
        Rp, tp = R.astype(per_point), t.astype(per_point)
        x = Rp[0, 0] * X + Rp[0, 1] * Y + Rp[0, 2] * Z + tp[0]
        y = Rp[1, 0] * X + Rp[1, 1] * Y + Rp[1, 2] * Z + tp[1]
        z = Rp[2, 0] * X + Rp[2, 1] * Y + Rp[2, 2] * Z + tp[2]
        iz = per_point(1) / z
        su = Kp[0, 0] * x + Kp[0, 1] * y
        sv = Kp[1, 1] * y
        r = np.stack([c[:, 3] - (su * iz + Kp[0, 2]), c[:, 4] - (sv * iz + Kp[1, 2])], 1)
        zero = np.zeros_like(x)
        du = np.stack([Kp[0, 0] * iz, Kp[0, 1] * iz, -su * iz * iz], 1)
        dv = np.stack([zero, Kp[1, 1] * iz, -sv * iz * iz], 1)
        J = np.empty((len(c), 2, 6), per_point)
        for row, g in ((0, du), (1, dv)):
            J[:, row, 0] = g[:, 2] * y - g[:, 1] * z
            J[:, row, 1] = g[:, 0] * z - g[:, 2] * x
            J[:, row, 2] = g[:, 1] * x - g[:, 0] * y
            J[:, row, 3:] = g
        J64, r64 = J.astype(np.float64), r.astype(np.float64)
        A = np.einsum("nri,nrj->ij", J64, J64)
        g = np.einsum("nri,nr->i", J64, r64)
        try:
            if not (np.all(np.isfinite(A)) and np.all(np.isfinite(g))):
                break
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            break
        d = np.linalg.solve(L.T, np.linalg.solve(L, g))
        E = _exp_so3(d[:3])
        R, t = E @ R, E @ t + d[3:]
    return R, t


def ransac(corr, K, R_ref, t_ref, b, hyps=100, thr=3.0, refine_iters=10, seed=0,
           per_point=np.float64):
    """The whole contract for one sample → dict(R, t, ok, inliers, winner, hyp, score)."""
    K = np.asarray(K, np.float64)
    hyp = hypotheses(corr, K, b, hyps, seed)
    sc, _ = score(corr, hyp["P"], hyp["valid"], thr)
    w = winner(sc)
    res = dict(R=np.asarray(R_ref), t=np.asarray(t_ref), ok=False, inliers=0, winner=w, hyp=hyp,
               score=sc)
    if len(corr) >= 4 and hyp["valid"][w] and sc[w] >= 4:
        inl = reproj_errors(corr, hyp["P"][w]) < thr
        R, t = refine(corr, inl, hyp["R"][w], hyp["t"][w], K, refine_iters, per_point)
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
            res.update(R=R, t=t, ok=True, inliers=int(sc[w]), inlier_mask=inl)
    return res


def contaminate(flow, points_valid, frac=0.3, seed=0):
    """Move ``frac`` of each sample's valid pixels by an offset of magnitude 10-40 px (far from the
    3 px threshold).  flow [B, 2, H, W], points_valid [B, H, W] bool → (flow', moved [B, H, W] bool)."""
    rng = np.random.default_rng(seed + 424243)
    out, moved = np.array(flow, np.float32), np.zeros(points_valid.shape, bool)
    B, _, H, W = out.shape
    for b in range(B):
        p = np.flatnonzero(points_valid[b].reshape(-1))
        if len(p) == 0:
            continue
        sel = rng.choice(p, size=int(round(frac * len(p))), replace=False)
        mag = rng.uniform(10.0, 40.0, len(sel))
        ang = rng.uniform(0.0, 2 * np.pi, len(sel))
        f = out[b].reshape(2, -1)
        f[0, sel] += (mag * np.cos(ang)).astype(np.float32)
        f[1, sel] += (mag * np.sin(ang)).astype(np.float32)
        moved[b].reshape(-1)[sel] = True
    return out, moved
