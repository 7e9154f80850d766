"""Test-side helper (not a test): a numpy float32 restatement of ``scflow_render``'s structure
(scflow_amd/csrc/render.hip) — margined, clamped face bboxes, 16×16 screen tiles, faces walked
256 at a time, a (depth bits ‖ face index) minimum per pixel, a per-wave minimum depth per image
— with switches that break it the way such a kernel goes wrong.  The CPU tests use it to show
that the scenes of ``tests/render_cases.py`` catch each of those faults: unbroken it meets the
per-pixel rule, and every fault makes a stated assertion fire (tests/test_render_cases_host.py).
It is not a reference: the oracle is ``oracle/render_oracle.py``.

Faults
* ``no_partial_tiles`` — S // 16 tiles per side: the last partial tile row and column are lost;
* ``clamp_short``      — the bbox clamps to S − 2: the last row and column are never tested;
* ``drop_last_chunk``  — the face loop stops before a last chunk of fewer than 256 faces;
* ``ties_high``        — equal depths resolve to the higher face index;
* ``range_leak``       — an image's face range runs to the end of the batch's packed faces;
* ``zmin_first_image`` — the wave-level minimum handles only the first image present in a wave.
"""
import numpy as np

RT, CHUNK, WAVE = 16, 256, 64
K_EPS = np.float32(1e-8)
F = np.float32


def project32(verts, R, t, K, S):
    """[V,3] float32 NDC + depth, the kernel's expression order (no contraction)."""
    v, R, t, K = (np.asarray(a, np.float32) for a in (verts, R, t, K))
    X = R[0, 0] * v[:, 0] + R[0, 1] * v[:, 1] + R[0, 2] * v[:, 2] + t[0]
    Y = R[1, 0] * v[:, 0] + R[1, 1] * v[:, 1] + R[1, 2] * v[:, 2] + t[1]
    Z = R[2, 0] * v[:, 0] + R[2, 1] * v[:, 1] + R[2, 2] * v[:, 2] + t[2]
    u = K[0, 0] * X / Z + K[0, 2]
    w = K[1, 1] * Y / Z + K[1, 2]
    c0 = F(0.5) * F(S - 1)
    return np.stack([-(u - c0) / c0, -(w - c0) / c0, Z], 1).astype(np.float32)


def _bary(px, py, p0, p1, p2):
    """bary_at on broadcastable float32 arrays: (b [.., 3], pz, inside)."""
    area0 = (p2[..., 0] - p0[..., 0]) * (p1[..., 1] - p0[..., 1]) - (p2[..., 1] - p0[..., 1]) * (p1[..., 0] - p0[..., 0])
    area = area0 + K_EPS

    def edge(a, b):
        return ((px - a[..., 0]) * (b[..., 1] - a[..., 1]) - (py - a[..., 1]) * (b[..., 0] - a[..., 0])) / area
    w0, w1, w2 = edge(p1, p2), edge(p2, p0), edge(p0, p1)
    t0, t1, t2 = w0 * p1[..., 2] * p2[..., 2], p0[..., 2] * w1 * p2[..., 2], p0[..., 2] * p1[..., 2] * w2
    den = np.maximum(t0 + t1 + t2, K_EPS)
    b = np.stack([t0 / den, t1 / den, t2 / den], -1)
    pz = b[..., 0] * p0[..., 2] + b[..., 1] * p1[..., 2] + b[..., 2] * p2[..., 2]
    inside = (b.min(-1) > 0) & (pz >= 0) & (np.abs(area0) > K_EPS)
    return b, pz, inside


def _bbox(p, S, fault):
    """face_bbox for [F, 3, 3] projected corners: (c_lo, c_hi, r_lo, r_hi, kept)."""
    hi = S - 2 if fault == "clamp_short" else S - 1
    pix = lambda x: ((F(1) - x) * F(S) - F(1)) * F(0.5)  # noqa: E731
    c_lo = np.maximum(np.floor(pix(p[..., 0].max(1))).astype(np.int64) - 1, 0)
    c_hi = np.minimum(np.ceil(pix(p[..., 0].min(1))).astype(np.int64) + 1, hi)
    r_lo = np.maximum(np.floor(pix(p[..., 1].max(1))).astype(np.int64) - 1, 0)
    r_hi = np.minimum(np.ceil(pix(p[..., 1].min(1))).astype(np.int64) + 1, hi)
    kept = ~(p[..., 2] <= 0).all(1) & (c_lo <= c_hi) & (r_lo <= r_hi)
    return c_lo, c_hi, r_lo, r_hi, kept


def rasterize(vproj, faces, face_img, n_img, S, fault=None):
    """render_tile_kernel + the geometric part of render_shade_kernel over a packed batch:
    dict(p2f [N,S,S] packed face index or −1, zbuf, bary)."""
    vproj = np.asarray(vproj, np.float32)
    faces, face_img = np.asarray(faces, np.int64), np.asarray(face_img, np.int64)
    p = vproj[faces]                                      # [F, 3, 3]
    c_lo, c_hi, r_lo, r_hi, kept = _bbox(p, S, fault)
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    zf = np.full((n_img, S, S), empty, np.uint64)
    tiles = S // RT if fault == "no_partial_tiles" else -(-S // RT)
    for n in range(n_img):
        fb = int(np.searchsorted(face_img, n, "left"))
        fe = len(faces) if fault == "range_leak" else int(np.searchsorted(face_img, n + 1, "left"))
        for ty in range(tiles):
            for tx in range(tiles):
                tx0, ty0 = tx * RT, ty * RT
                r = ty0 + np.arange(RT * RT) // RT
                c = tx0 + np.arange(RT * RT) % RT
                px = F(1) - (2 * c + 1).astype(np.float32) / F(S)
                py = F(1) - (2 * r + 1).astype(np.float32) / F(S)
                best = np.full(RT * RT, empty, np.uint64)
                for f0 in range(fb, fe, CHUNK):
                    if fault == "drop_last_chunk" and f0 + CHUNK > fe:
                        break
                    f = np.arange(f0, min(f0 + CHUNK, fe))
                    f = f[kept[f] & (c_hi[f] >= tx0) & (c_lo[f] < tx0 + RT) & (r_hi[f] >= ty0) & (r_lo[f] < ty0 + RT)]
                    if not len(f):
                        continue
                    b, pz, inside = _bary(px[None], py[None], p[f, 0][:, None], p[f, 1][:, None], p[f, 2][:, None])
                    inbox = (c[None] >= c_lo[f, None]) & (c[None] <= c_hi[f, None]) & \
                            (r[None] >= r_lo[f, None]) & (r[None] <= r_hi[f, None])
                    low = (np.uint64(0xFFFFFFFF) - f.astype(np.uint64)) if fault == "ties_high" else f.astype(np.uint64)
                    key = (pz.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[:, None]
                    key = np.where(inside & inbox, key, empty)
                    best = np.minimum(best, key.min(0))
                ok = (r < S) & (c < S)
                zf[n, r[ok], c[ok]] = best[ok]
    hit = zf != empty
    low = (zf & np.uint64(0xFFFFFFFF)).astype(np.int64)
    fwin = np.where(hit, (0xFFFFFFFF - low) if fault == "ties_high" else low, 0)
    rr, cc = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    px = (F(1) - (2 * cc + 1).astype(np.float32) / F(S))[None]
    py = (F(1) - (2 * rr + 1).astype(np.float32) / F(S))[None]
    pw = p[fwin]                                          # [N, S, S, 3, 3]
    b, pz, _ = _bary(px, py, pw[..., 0, :], pw[..., 1, :], pw[..., 2, :])
    return dict(p2f=np.where(hit, fwin, -1), zbuf=np.where(hit, pz, F(-1)).astype(np.float32),
                bary=np.where(hit[..., None], b, F(-1)).astype(np.float32))


def zmin_per_image(z, vert_img, n_img, fault=None):
    """render_project_kernel's minimum depth per image: per 64-lane wave, one reduction per image
    present in the wave, then a minimum across waves.  Untouched images keep the fill value."""
    z, vert_img = np.asarray(z, np.float32), np.asarray(vert_img, np.int64)
    out = np.full(n_img, np.frombuffer(b"\x7f" * 4, np.float32)[0], np.float32)
    for w0 in range(0, len(z), WAVE):
        zi, ni = z[w0:w0 + WAVE], vert_img[w0:w0 + WAVE]
        for n in (ni[:1] if fault == "zmin_first_image" else np.unique(ni)):
            m = zi[(ni == n) & (zi > 0)]
            if len(m):
                out[n] = min(out[n], m.min())
    return out


def light_location(zmin, R, light):
    """light_of for (seperate_lights, default_lights) → [N, 3] float32."""
    seps, deflt = light
    R = np.asarray(R, np.float32)
    if seps:
        lz = np.maximum(zmin - F(400), F(0))
    elif deflt:
        return np.tile(np.array([0, 1, 0], np.float32), (len(zmin), 1))
    else:
        lz = np.full(len(zmin), np.floor(zmin.min() / F(100)) * F(100) / F(4), np.float32)
    return R[:, :, 2] * lz[:, None]


def render_batch(b, fault=None, light=(True, True)):
    """A tests/render_cases.py batch through the restatement: (batch arrays with packed
    pix_to_face, light locations [N, 3])."""
    n = len(b["names"])
    ms = [b["meshes"][i] for i in range(n)]
    nv, nf = [len(m[0]) for m in ms], [len(m[1]) for m in ms]
    voff = np.concatenate([[0], np.cumsum(nv)[:-1]])
    vproj = np.concatenate([project32(m[0], b["R"][i], b["t"][i], b["K"][i], b["S"]) for i, m in enumerate(ms)])
    faces = np.concatenate([m[1] + o for m, o in zip(ms, voff)])
    vert_img, face_img = np.repeat(np.arange(n), nv), np.repeat(np.arange(n), nf)
    out = rasterize(vproj, faces, face_img, n, b["S"], fault)
    zmin = zmin_per_image(vproj[:, 2], vert_img, n, fault)
    return out, light_location(zmin, b["R"], light)
