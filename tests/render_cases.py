"""Test-side helper (not a test): the meshes, scenes and the per-pixel comparison rule that the
renderer's CPU and GPU tests share (``tests/test_render_cases_host.py``,
``tests/test_gpu_render.py``).  numpy + the CPU oracle (``oracle/render_oracle.py``); no GPU.

Scenes (``batch(name, seed)``, two seeds each; rotations from a seeded QR with determinant +1;
every vertex at view depth Z > 0):

* ``s40`` — S = 40 (2.5 tiles of 16 per side), five images with five vertex / face counts:
  ``border`` (centre outside the image, silhouette across two borders), ``closeup`` (every pixel
  covered), ``bigbox`` (12 faces, each wider than a tile), ``needle`` (sliver triangles, < 5 %
  covered), ``offscreen`` (nothing covered);
* ``s24`` — S = 24 (1.5 tiles), seven images: box / tetra / 6×8 ellipsoid / box / octa / box with
  8, 4, 42, 8, 6, 8 vertices (five images in the projection kernel's first 64-lane wave), view
  depths 520, 610, 700, 350, 450, 900 (350: the separate light clamps to 0; the batch minimum is
  in the middle), and ``far``: a 10×16 ellipsoid at 3000 that lands inside a 3×3 pixel block;
* ``torus56`` — S = 56, a torus: self-occlusion, background inside the mesh's bbox;
* ``double48`` — S = 48, two interpenetrating ellipsoids with the first one's faces appended a
  second time: exact depth ties against higher face indices;
* ``chunks72`` — S = 72 (4.5 tiles), 1728 faces = seven 256-face chunks, across a border.

The rule (``compare_with_oracle``).  The kernel's face g and the fp64 oracle's face o at a pixel
may differ only where both of these hold, every face evaluated in fp64 with the oracle's formulas:

* g = −1, or g is a legitimate contender there: its three corrected barycentrics ≥ −δ, pz ≥ 0;
* o = −1, or o could legitimately lose: its smallest barycentric ≤ δ (the pixel centre is on an
  edge), or |pz_g − pz_o| ≤ ε·pz_o (a depth near-tie, e.g. an interpenetration line).

δ = 1e-3 and ε = 1e-5 are the barycentric and zbuf tolerances of ``test_gpu_render.py``.  A
differing pixel that does not meet the rule is *unexplained*: none are allowed.  Explained pixels
are left out of the value comparison and capped per image at max(2, 0.1 % of S²).  Everywhere
else: zbuf rtol 1e-5, barycentrics atol 1e-3, RGBA atol 2e-3 on covered pixels; background RGBA,
zbuf −1, pix_to_face −1 and bary −1 exact.

The cap is four or more times what the reference needs: the float32 oracle against the float64
oracle (CPU, ``test_render_cases_host.py``) differs on 0 pixels of every scene and seed (largest
differences on the same-face pixels: zbuf 9.5e-7 relative, barycentrics 3.3e-5, RGBA 5.5e-6), and
that test holds it to a quarter of the cap.  The HIP kernel on the MI355X
(``test_gpu_render.py``): 0 differing pixels on all 109 rendered images of these scenes and on
the 20 images of the ``make_scene`` cases; largest differences zbuf 6.2e-7 / 2.8e-6 relative,
barycentrics 3.6e-5 / 6.7e-4, RGBA 6.4e-6 / 1.7e-5 (edge scenes / ``make_scene`` at S = 128).
"""
from functools import lru_cache
import math

import numpy as np
import torch

from scflow_amd import synthetic

DELTA = 1e-3      # barycentric tolerance (test_gpu_render.py)
EPS_Z = 1e-5      # relative zbuf tolerance (test_gpu_render.py)
RGB_ATOL = 2e-3
K_EPS = 1e-8      # the rasteriser's kEpsilon (oracle/render_oracle.py)
TILE = 16         # render_tile_kernel's screen tile
SEEDS = (0, 1)
BATCHES = ("s40", "s24", "torus56", "double48", "chunks72")
LIGHTS = ((True, True), (False, True), (True, False), (False, False))  # (seperate, default)


# ------------------------------------------------------------------------------------ meshes
def _colors(verts):
    """A smooth vertex-colour pattern in [0.1, 0.9]."""
    u = verts / np.abs(verts).max(0, keepdims=True).clip(1e-9)
    return (0.5 + 0.4 * np.stack([u[:, 0], u[:, 1] * u[:, 2], np.cos(3 * u[:, 0])], 1)).astype(np.float32)


def _mesh(verts, faces):
    verts = np.asarray(verts, np.float64)
    return verts.astype(np.float32), np.asarray(faces, np.int64), _colors(verts)


def box(hx, hy, hz):
    """8 vertices, 12 faces, outward winding."""
    v = [[sx * hx, sy * hy, sz * hz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)]
    # vertex index = 4·(z > 0) + 2·(y > 0) + (x > 0)
    f = [[0, 2, 3], [0, 3, 1],   # z = −hz
         [4, 5, 7], [4, 7, 6],   # z = +hz
         [0, 1, 5], [0, 5, 4],   # y = −hy
         [2, 6, 7], [2, 7, 3],   # y = +hy
         [0, 4, 6], [0, 6, 2],   # x = −hx
         [1, 3, 7], [1, 7, 5]]   # x = +hx
    return _mesh(v, f)


def tetra(s=50.0):
    """4 vertices, 4 faces, outward winding."""
    v = s * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    return _mesh(v, [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def octa(s=55.0):
    """6 vertices (±s on each axis), 8 faces, outward winding."""
    v = s * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return _mesh(v, f)


def torus(R0, r0, nu, nv):
    """nu·nv vertices, 2·nu·nv faces, outward winding; the axis is z."""
    v = []
    for i in range(nu):
        u = 2 * math.pi * i / nu
        for j in range(nv):
            w = 2 * math.pi * j / nv
            v.append([(R0 + r0 * math.cos(w)) * math.cos(u), (R0 + r0 * math.cos(w)) * math.sin(u),
                      r0 * math.sin(w)])
    idx = lambda i, j: (i % nu) * nv + (j % nv)  # noqa: E731
    f = []
    for i in range(nu):
        for j in range(nv):
            f.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
            f.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
    return _mesh(v, f)


def double_ellipsoid(semi=(60.0, 46.0, 36.0)):
    """A 12×16 ellipsoid, a copy with permuted axes that interpenetrates it, and the first one's
    faces once more at the end of the face array (exact depth ties against higher indices).
    Returns the mesh and (faces of the first, faces of the second)."""
    v, f, c = synthetic.ellipsoid_mesh(np.array(semi), 12, 16)
    v2 = np.ascontiguousarray(v[:, [1, 2, 0]])
    verts = np.concatenate([v, v2])
    faces = np.concatenate([f, f + len(v), f])
    return (verts, faces, np.concatenate([c, c])), (len(f), len(f))


def rotation(seed):
    """A seeded QR rotation, determinant +1 (float64)."""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)


def _ell(semi, n_lat, n_lon):
    return synthetic.ellipsoid_mesh(np.array(semi, np.float64), n_lat, n_lon)


# ------------------------------------------------------------------------------------ scenes
def _images(name):
    """[(image name, mesh, t, K)] of a batch."""
    if name == "s40":
        return [("border", _ell((60, 46, 36), 20, 32), (60, -45, 700), _K(300, 260, 17.3, 23.9)),
                ("closeup", _ell((100, 76, 60), 24, 40), (0, 0, 400), _K(400, 380, 20, 19)),
                ("bigbox", box(60, 50, 40), (4, -3, 260), _K(110, 100, 19, 21)),
                ("needle", _ell((100, 6, 6), 16, 24), (0, 0, 500), _K(90, 95, 20, 20)),
                ("offscreen", _ell((60, 46, 36), 8, 12), (900, 0, 700), _K(200, 200, 19.5, 19.5))]
    if name == "s24":
        ms = [("box0", box(45, 35, 25)), ("tetra", tetra()), ("ell6x8", _ell((50, 38, 30), 6, 8)),
              ("box350", box(40, 30, 22)), ("octa", octa(40.0)), ("box900", box(60, 45, 30))]
        out = []
        for i, ((nm, m), tz) in enumerate(zip(ms, (520, 610, 700, 350, 450, 900))):
            out.append((nm, m, (3.0 * i - 6.0, 5.0 - 2.0 * i, tz),
                        _K(0.2 * tz, 0.22 * tz, 11.5 + 0.17 * (i - 2), 11.5 - 0.23 * (i - 3))))
        # pixel 12's centre is OpenCV 12.5·23/24
        out.append(("far", _ell((50, 38, 30), 10, 16), (0, 0, 3000), _K(90, 90, 12.5 * 23 / 24, 12.5 * 23 / 24)))
        return out
    if name == "torus56":
        return [("torus", torus(60, 22, 24, 16), (10, 5, 600), _K(200, 210, 27.5, 27.5))]
    if name == "double48":
        return [("double", double_ellipsoid()[0], (0, 0, 600), _K(220, 220, 23.5, 23.5))]
    if name == "chunks72":
        return [("chunks", _ell((60, 46, 36), 28, 32), (-70, 60, 650), _K(330, 300, 30, 40))]
    raise KeyError(name)


# rotation seed of image i of a batch = ROT_SEEDS[batch][seed] + i (poses chosen so that every
# scene has its property: tests/test_render_cases_host.py; the torus is seen edge-on, hole hidden,
# with the first seed and at a slant with its hole open with the second;
# chunks72 shows faces of its last, partial 256-face chunk with both)
ROT_SEEDS = {"s40": (1, 7), "s24": (20, 40), "torus56": (7, 3), "double48": (30, 31), "chunks72": (50, 54)}
SIZES = {"s40": 40, "s24": 24, "torus56": 56, "double48": 48, "chunks72": 72}


@lru_cache(maxsize=None)
def batch(name, seed):
    """dict: S, names, labels [N] int64 (label i = image i), meshes {label: (verts, faces,
    colors)}, R [N,3,3] / t [N,3] / K [N,3,3] float32, face_offset [N+1].  Read-only."""
    ims = _images(name)
    n = len(ims)
    R = np.stack([rotation(ROT_SEEDS[name][seed] + i) for i in range(n)]).astype(np.float32)
    t = np.array([im[2] for im in ims], np.float32)
    K = np.stack([im[3] for im in ims]).astype(np.float32)
    meshes = {i: im[1] for i, im in enumerate(ims)}
    off = np.concatenate([[0], np.cumsum([len(im[1][1]) for im in ims])]).astype(np.int64)
    out = dict(S=SIZES[name], names=[im[0] for im in ims], labels=np.arange(n, dtype=np.int64),
               meshes=meshes, R=R, t=t, K=K, face_offset=off)
    for a in (R, t, K, off, out["labels"]):
        a.setflags(write=False)
    for m in meshes.values():
        for a in m:
            a.setflags(write=False)
    return out


def _torch_meshes(meshes, dtype):
    return {lab: (torch.from_numpy(np.array(v)).to(dtype), torch.from_numpy(np.array(f)),
                  torch.from_numpy(np.array(c)).to(dtype)) for lab, (v, f, c) in meshes.items()}


def run_oracle(meshes, R, t, K, labels, S, light, dtype=torch.float64):
    """``oracle.render_oracle.render`` on the fp32-rounded inputs in ``dtype``, split per image:
    list of dict(p2f [S,S] int64 local face index, zbuf, bary, images) numpy arrays."""
    import oracle.render_oracle as ro
    T = lambda a: torch.from_numpy(np.array(a)).to(dtype)  # noqa: E731
    imgs, zbuf, p2f, bary = ro.render(_torch_meshes(meshes, dtype), T(R), T(t), T(K),
                                      [int(x) for x in labels], S, light=light)
    off = np.concatenate([[0], np.cumsum([len(meshes[int(lab)][1]) for lab in labels])])
    return split_batch(dict(p2f=p2f.numpy(), zbuf=zbuf.numpy(), bary=bary.numpy(), images=imgs.numpy()), off)


def split_batch(b, face_offset):
    """Batch arrays (packed pix_to_face) → per-image dicts with local face indices."""
    out = []
    for i in range(b["p2f"].shape[0]):
        p = np.asarray(b["p2f"][i]).astype(np.int64)
        d = dict(p2f=np.where(p >= 0, p - int(face_offset[i]), p), zbuf=np.asarray(b["zbuf"][i]),
                 bary=np.asarray(b["bary"][i]))
        if b.get("images") is not None:
            d["images"] = np.asarray(b["images"][i])
        out.append(d)
    return out


@lru_cache(maxsize=None)
def oracle(name, seed, light=(True, True), fp32=False):
    """The batch through the oracle (fp64, or the float32 stand-in): per-image dicts, shared."""
    b = batch(name, seed)
    return run_oracle(b["meshes"], b["R"], b["t"], b["K"], b["labels"], b["S"], light,
                      torch.float32 if fp32 else torch.float64)


def project64(verts, R, t, K, S):
    """fp64 NDC + view depth [V,3] of the fp32-rounded inputs (the oracle's projection)."""
    import oracle.render_oracle as ro
    T = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
    return ro.project_ndc(T(verts), T(R), T(t), T(K), S).numpy()


@lru_cache(maxsize=None)
def ndc64(name, seed):
    b = batch(name, seed)
    return [project64(b["meshes"][i][0], b["R"][i], b["t"][i], b["K"][i], b["S"])
            for i in range(len(b["names"]))]


@lru_cache(maxsize=None)
def lights64(name, seed, light):
    import oracle.render_oracle as ro
    b = batch(name, seed)
    T = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
    return ro.light_location([T(b["meshes"][i][0]) for i in range(len(b["names"]))], T(b["R"]),
                             T(b["t"]), light).numpy()


# ------------------------------------------------------------------------------------ the rule
def eval_faces(ndc, faces, f, r, c, S):
    """Faces ``f`` [n] at pixels (r, c) [n] in fp64 with the oracle's formulas: corrected
    barycentrics [n,3], pz [n], and whether the face is non-degenerate (|area| > 1e-8)."""
    ndc = np.asarray(ndc, np.float64)
    f = np.asarray(f, np.int64)
    v0, v1, v2 = (ndc[faces[f, k]] for k in range(3))
    px = 1.0 - (2.0 * np.asarray(c, np.float64) + 1.0) / S
    py = 1.0 - (2.0 * np.asarray(r, np.float64) + 1.0) / S

    def edge(a, b):
        return (px - a[:, 0]) * (b[:, 1] - a[:, 1]) - (py - a[:, 1]) * (b[:, 0] - a[:, 0])
    area0 = (v2[:, 0] - v0[:, 0]) * (v1[:, 1] - v0[:, 1]) - (v2[:, 1] - v0[:, 1]) * (v1[:, 0] - v0[:, 0])
    area = area0 + K_EPS
    w0, w1, w2 = edge(v1, v2) / area, edge(v2, v0) / area, edge(v0, v1) / area
    t0, t1, t2 = w0 * v1[:, 2] * v2[:, 2], v0[:, 2] * w1 * v2[:, 2], v0[:, 2] * v1[:, 2] * w2
    den = np.maximum(t0 + t1 + t2, K_EPS)
    b = np.stack([t0 / den, t1 / den, t2 / den], 1)
    pz = (b * np.stack([v0[:, 2], v1[:, 2], v2[:, 2]], 1)).sum(1)
    return b, pz, np.abs(area0) > K_EPS


def cap(S):
    """Explained pixels allowed per image."""
    return max(2.0, 0.001 * S * S)


def compare_with_oracle(got, oracle, ndc64, faces, S):
    """One image.  ``got`` / ``oracle``: dict(p2f [S,S] local face index or −1, zbuf [S,S],
    bary [S,S,3], images [S,S,4] or absent); ``ndc64`` [V,3] the fp64 projection; ``faces``
    [F,3].  Applies the per-pixel rule (module docstring) and returns the figures: mismatches,
    explained, unexplained (with their pixels), the largest zbuf (relative), barycentric and
    RGBA differences on the pixels with the same face, and whether the background is exact."""
    faces = np.asarray(faces, np.int64)
    g, o = np.asarray(got["p2f"], np.int64), np.asarray(oracle["p2f"], np.int64)
    assert g.shape == o.shape == (S, S)
    assert g.min() >= -1 and g.max() < len(faces)
    rr, cc = np.nonzero(g != o)
    gf, of = g[rr, cc], o[rr, cc]
    n = len(rr)
    ok_g, ok_o = np.ones(n, bool), np.ones(n, bool)
    pz_g = np.full(n, np.nan)
    hg, ho = gf >= 0, of >= 0
    if hg.any():
        b, pz, nd = eval_faces(ndc64, faces, gf[hg], rr[hg], cc[hg], S)
        ok_g[hg] = (b.min(1) >= -DELTA) & (pz >= 0) & nd
        pz_g[hg] = pz
    if ho.any():
        b, pz, _ = eval_faces(ndc64, faces, of[ho], rr[ho], cc[ho], S)
        with np.errstate(invalid="ignore"):
            tie = np.abs(pz_g[ho] - pz) <= EPS_Z * pz   # False where g = −1 (nan)
        ok_o[ho] = (b.min(1) <= DELTA) | tie
    explained = ok_g & ok_o
    same = g == o
    hit = same & (o >= 0)
    bg = same & (o < 0)
    st = dict(mismatch=n, explained=int(explained.sum()), unexplained=int((~explained).sum()),
              unexplained_pixels=[(int(r), int(c), int(a), int(b_)) for r, c, a, b_, e in
                                  zip(rr, cc, gf, of, explained) if not e][:8],
              covered=int((o >= 0).sum()), same_face=int(hit.sum()), dz=0.0, dbary=0.0, drgb=0.0)
    gz, oz = np.asarray(got["zbuf"], np.float64), np.asarray(oracle["zbuf"], np.float64)
    gb, ob = np.asarray(got["bary"], np.float64), np.asarray(oracle["bary"], np.float64)
    if hit.any():
        st["dz"] = float((np.abs(gz[hit] - oz[hit]) / np.abs(oz[hit])).max())
        st["dbary"] = float(np.abs(gb[hit] - ob[hit]).max())
    st["bg_exact"] = bool((gz[bg] == -1).all() and (gb[bg] == -1).all())
    # a covered pixel never carries the background's markers
    st["fg_marked"] = bool((gz[g >= 0] >= 0).all()) and bool((gz[g < 0] == -1).all())
    if got.get("images") is not None:
        gi, oi = np.asarray(got["images"], np.float64), np.asarray(oracle["images"], np.float64)
        if hit.any():
            st["drgb"] = float(np.abs(gi[hit] - oi[hit]).max())
        st["bg_exact"] = st["bg_exact"] and bool((gi[bg] == oi[bg]).all())
        st["fg_marked"] = st["fg_marked"] and bool((gi[g >= 0][:, 3] == 1).all()) and \
            bool((gi[g < 0][:, 3] == 0).all())
    return st


def describe(tag, st):
    return (f"{tag}: covered {st['covered']}, mismatch {st['mismatch']} (explained "
            f"{st['explained']}, unexplained {st['unexplained']}), max zbuf rel {st['dz']:.2e}, "
            f"bary {st['dbary']:.2e}, rgba {st['drgb']:.2e}")


def assert_stats(tag, st, S, cap_fraction=1.0):
    """The assertions of the rule on one image's figures."""
    assert st["unexplained"] == 0, (tag, st["unexplained_pixels"])
    assert st["explained"] <= cap_fraction * cap(S), (tag, st["explained"], cap(S))
    assert st["dz"] <= EPS_Z, (tag, st["dz"])
    assert st["dbary"] <= DELTA, (tag, st["dbary"])
    assert st["drgb"] <= RGB_ATOL, (tag, st["drgb"])
    assert st["bg_exact"] and st["fg_marked"], tag


def compare_batch(tag, got, orc, ndcs, meshes, labels, S, cap_fraction=1.0, names=None):
    """compare_with_oracle + assert_stats on every image of a batch (per-image dict lists);
    prints each image's figures first.  Returns the per-image figures."""
    stats = []
    for i, lab in enumerate(labels):
        st = compare_with_oracle(got[i], orc[i], ndcs[i], meshes[int(lab)][1], S)
        print(describe(f"{tag}[{names[i] if names else i}]", st))
        stats.append(st)
    for i, st in enumerate(stats):
        assert_stats(f"{tag}[{names[i] if names else i}]", st, S, cap_fraction)
    return stats
