"""Test-side helper (not a test): scene visibility (include/scflow_hip.h
``scflow_scene_visibility``) restated in numpy with per-instance, per-face loops.  It shares no code
with the product.  ``dtype`` float64 is the reference; float32 is the stand-in that shows what
rounding alone can change.

Besides the call's outputs it returns, per instance and pixel, how far every decision was from
flipping:

* ``edge_margin`` [n, Hc, Wc] (canvas, px): over the instance's non-dropped faces, the smallest
  |min_i s_i|, s_i the signed distance from the sample to the line of edge i (positive inside).
  A face contains the sample ⇔ min_i s_i > 0, so this is the distance to the nearest edge line of
  a face that (nearly) contains it; inf where no face is within a pixel.
* ``decision_margin`` [n, H, W] (mm): the smallest of |M − T − delta| (the visibility test, where
  T > 0; without a sensor depth not for the nearest instance, whose M is T itself), T (the T = 0 test, where a sensor depth is given and T > 0) and, where more than one
  instance is visible, the gap between the two smallest *different* distances (the nearest-instance
  choice; equal distances — a duplicate pose — go to the lower index in every precision).
* ``edge_thr`` [n] and ``dec_thr`` [F]: 64·2⁻²³·max(|u|, |v|, W, H) over the instance's projected
  vertices, and 64·2⁻²³·(the largest distance in the frame).
"""
import numpy as np

ULP64 = 64.0 * 2.0 ** -23


def scene_visibility(meshes, labels, frame_index, R, t, K, H, W, depth_test=None, delta=15.0,
                     margin=(0, 0), pixel_offset=0.0, dtype=np.float64):
    """meshes {label: (verts [V,3], faces [F,3], …)}; labels / frame_index [n] (any order); R
    [n,3,3], t [n,3], K [F,3,3]; depth_test [F,H,W] or None; margin (x, y)."""
    dt = dtype
    n, F = len(labels), len(K)
    mx, my = int(margin[0]), int(margin[1])
    Wc, Hc = W + 2 * mx, H + 2 * my
    off = dt(pixel_offset)
    depth_c = np.full((n, Hc, Wc), np.inf, dt)            # instance depth on the canvas
    edge_margin = np.full((n, Hc, Wc), np.inf)
    edge_thr = np.full(n, ULP64 * max(W, H))
    skipped = np.zeros(n, bool)
    for i in range(n):
        lab, f = int(labels[i]), int(frame_index[i])
        m = meshes.get(lab)
        if m is None or len(m[0]) == 0 or len(m[1]) == 0 or f < 0 or f >= F:
            skipped[i] = True
            continue
        Kf = np.asarray(K[f], dt)
        fx, fy, cx, cy = Kf[0, 0], Kf[1, 1], Kf[0, 2], Kf[1, 2]
        X = np.asarray(m[0], dt) @ np.asarray(R[i], dt).T + np.asarray(t[i], dt)
        Z = X[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = fx * X[:, 0] / Z + cx
            v = fy * X[:, 1] / Z + cy
        front = Z > 0
        if front.any():
            edge_thr[i] = ULP64 * max(float(np.abs(u[front]).max()), float(np.abs(v[front]).max()), W, H)
        for face in np.asarray(m[1], np.int64):
            if not front[face].all():
                continue                                   # dropped: a vertex at Z ≤ 0
            (x0, x1, x2), (y0, y1, y2), (z0, z1, z2) = u[face], v[face], Z[face]
            area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
            if area == 0:
                continue                                   # dropped: zero screen area
            # the canvas pixels within a pixel of the face's box
            c0 = max(int(np.floor(min(x0, x1, x2) - off)) - 1, -mx)
            c1 = min(int(np.ceil(max(x0, x1, x2) - off)) + 1, W + mx - 1)
            r0 = max(int(np.floor(min(y0, y1, y2) - off)) - 1, -my)
            r1 = min(int(np.ceil(max(y0, y1, y2) - off)) + 1, H + my - 1)
            if c0 > c1 or r0 > r1:
                continue
            px = (np.arange(c0, c1 + 1).astype(dt) + off)[None, :]
            py = (np.arange(r0, r1 + 1).astype(dt) + off)[:, None]
            sgn = dt(1.0) if area > 0 else dt(-1.0)
            e0 = sgn * ((x1 - px) * (y2 - py) - (y1 - py) * (x2 - px))
            e1 = sgn * ((x2 - px) * (y0 - py) - (y2 - py) * (x0 - px))
            e2 = sgn * ((x0 - px) * (y1 - py) - (y0 - py) * (x1 - px))
            a = abs(area)
            w0, w1, w2 = e0 / a, e1 / a, e2 / a
            inside = (e0 > 0) & (e1 > 0) & (e2 > 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                z = 1 / (w0 / z0 + w1 / z1 + w2 / z2)
            win = (slice(r0 + my, r1 + my + 1), slice(c0 + mx, c1 + mx + 1))
            d = depth_c[i][win]
            depth_c[i][win] = np.where(inside & (z < d), z, d)
            s = np.minimum(np.minimum(e0 / np.hypot(x2 - x1, y2 - y1), e1 / np.hypot(x0 - x2, y0 - y2)),
                           e2 / np.hypot(x1 - x0, y1 - y0))
            edge_margin[i][win] = np.minimum(edge_margin[i][win], np.abs(s.astype(np.float64)))

    cov_c = np.isfinite(depth_c)
    depth_inst = np.where(cov_c, depth_c, 0)[:, my:my + H, mx:mx + W].astype(dt)
    cov = depth_inst > 0
    # distances
    ys, xs = np.mgrid[0:H, 0:W]
    M = np.zeros((n, H, W), dt)
    Tm = np.zeros((F, H, W), dt)
    factor = np.zeros((F, H, W), dt)
    for f in range(F):
        Kf = np.asarray(K[f], dt)
        factor[f] = np.sqrt(((xs.astype(dt) - Kf[0, 2]) / Kf[0, 0]) ** 2 +
                            ((ys.astype(dt) - Kf[1, 2]) / Kf[1, 1]) ** 2 + 1)
    for i in range(n):
        if not skipped[i]:
            M[i] = depth_inst[i] * factor[int(frame_index[i])]
    for f in range(F):
        if depth_test is not None:
            Tm[f] = np.asarray(depth_test[f], dt) * factor[f]
        else:
            mine = [i for i in range(n) if not skipped[i] and int(frame_index[i]) == f]
            if mine:
                stack = np.where(cov[mine], M[mine], np.inf).min(0)
                Tm[f] = np.where(np.isfinite(stack), stack, 0)
    dl = dt(delta)
    vis = np.zeros((n, H, W), bool)
    valid = np.zeros((n, H, W), bool)
    dec = np.full((n, H, W), np.inf)
    dec_thr = np.zeros(F)
    for f in range(F):
        far = float(Tm[f].max())
        for i in range(n):
            if not skipped[i] and int(frame_index[i]) == f and cov[i].any():
                far = max(far, float(M[i].max()))
        dec_thr[f] = ULP64 * far
    for i in range(n):
        if skipped[i]:
            continue
        T = Tm[int(frame_index[i])]
        vis[i] = cov[i] & ((T == 0) | (M[i] - T <= dl))
        valid[i] = cov[i] & (T > 0)
        g = np.where(cov[i] & (T > 0), np.abs((M[i] - T - dl).astype(np.float64)), np.inf)
        if depth_test is None:
            # T is the nearest instance's own M: M − T = 0 there in every precision, no decision
            g = np.where(M[i] == T, np.inf, g)
        else:
            g = np.minimum(g, np.where(cov[i] & (T > 0), T.astype(np.float64), np.inf))
        dec[i] = g
    inst_id = np.full((F, H, W), -1, np.int32)
    depth_scene = np.zeros((F, H, W), dt)
    for f in range(F):
        mine = [i for i in range(n) if not skipped[i] and int(frame_index[i]) == f]
        if not mine:
            continue
        dz = np.where(cov[mine], depth_inst[mine], np.inf).min(0)
        depth_scene[f] = np.where(np.isfinite(dz), dz, 0)
        best = np.full((H, W), np.inf)
        second = np.full((H, W), np.inf)      # the smallest distance different from the best
        for i in mine:                        # ascending index: a tie keeps the lower one
            Mi = np.where(vis[i], M[i].astype(np.float64), np.inf)
            better = Mi < best
            second = np.where(better, best, np.where((Mi > best) & (Mi < second), Mi, second))
            inst_id[f] = np.where(better, i, inst_id[f])
            best = np.where(better, Mi, best)
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isfinite(second), second - best, np.inf)
        for i in mine:
            dec[i] = np.where(vis[i], np.minimum(dec[i], gap), dec[i])

    stats = np.zeros((n, 12), np.int32)
    for i in range(n):
        def box(mask, ox, oy):
            rr, cc = np.nonzero(mask)
            if len(rr) == 0:
                return [-1, -1, -1, -1]
            return [int(cc.min()) - ox, int(rr.min()) - oy, int(cc.max() - cc.min()) + 1,
                    int(rr.max() - rr.min()) + 1]
        stats[i, 0] = cov_c[i].sum()
        stats[i, 1] = valid[i].sum()
        stats[i, 2] = vis[i].sum()
        stats[i, 3:7] = box(cov_c[i], mx, my)
        stats[i, 7:11] = box(vis[i], 0, 0)
    return dict(stats=stats, inst_id=inst_id, depth_scene=depth_scene, depth_inst=depth_inst,
                mask_visib=vis.astype(np.uint8), cover_canvas=cov_c, edge_margin=edge_margin,
                decision_margin=dec, edge_thr=edge_thr, dec_thr=dec_thr, skipped=skipped)


def ambiguous(res, frame_index, F, margin=(0, 0)):
    """(frame [F, H, W] bool, canvas [F, Hc, Wc] bool): the pixels ambiguous for any instance of
    the frame — an edge margin below the instance's ``edge_thr`` or, in the frame, a decision
    margin below the frame's ``dec_thr``.  On the canvas outside the frame only the edges count."""
    n, Hc, Wc = res["edge_margin"].shape
    mx, my = int(margin[0]), int(margin[1])
    H, W = Hc - 2 * my, Wc - 2 * mx
    canvas = np.zeros((F, Hc, Wc), bool)
    for i in range(n):
        f = int(frame_index[i])
        if res["skipped"][i]:
            continue
        canvas[f] |= res["edge_margin"][i] < res["edge_thr"][i]
        canvas[f, my:my + H, mx:mx + W] |= res["decision_margin"][i] < res["dec_thr"][f]
    return canvas[:, my:my + H, mx:mx + W].copy(), canvas
