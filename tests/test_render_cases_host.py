"""CPU: the renderer's edge scenes (tests/render_cases.py) have the properties they were built
for, and the per-pixel rule, its cap and the value tolerances are satisfiable by the reference
alone — the float32 oracle stands in for the kernel against the float64 oracle on the same
fp32-rounded inputs.  The stand-in must stay at 0 unexplained pixels and within a quarter of the
kernel's cap on explained ones.

Measured here (float32 oracle vs float64 oracle, both seeds, all scenes, the four light settings
on s40 and s24: 102 images): 0 differing pixels on every image; on the pixels with the same face
the largest differences are zbuf 9.5e-7 relative, barycentrics 3.3e-5, RGBA 5.5e-6 (bounds 1e-5,
1e-3, 2e-3).

The last part shows that the scenes catch a broken kernel without running one on a GPU: a numpy
float32 restatement of the kernel's structure (tests/render_restatement.py) meets the rule with 0
differing pixels when unbroken, and each of its faults trips an assertion that
``test_render_edge_scenes`` makes — a lost partial tile row / column and a bbox clamped one pixel
short leave unexplained pixels on ``closeup`` / ``border`` / ``chunks72``, a dropped last face
chunk on ``chunks72`` and ``closeup``, a face range that leaks into the next image is caught on
s24 / s40, ties to the higher index exceed the cap on explained pixels and land in
``double_ellipsoid``'s repeated face block, and a wave-level minimum that serves one image per
wave moves the lights of s24.
"""
import numpy as np
import pytest

from tests import render_cases as rc

ro = pytest.importorskip("oracle.render_oracle")

ALL = [(n, s) for n in rc.BATCHES for s in rc.SEEDS]


def _image(name, seed, which):
    b = rc.batch(name, seed)
    i = b["names"].index(which)
    return b, i, rc.oracle(name, seed)[i], rc.ndc64(name, seed)[i]


def _cover(o):
    return o["p2f"] >= 0


def _pixel_bbox(ndc, faces, S):
    """Unmargined pixel bbox [F, 4] (c_lo, c_hi, r_lo, r_hi) of every face, clamped to the image."""
    p = ndc[faces]                                       # [F, 3, 3]
    to_pix = lambda x: ((1.0 - x) * S - 1.0) * 0.5       # noqa: E731
    c_lo, c_hi = np.floor(to_pix(p[..., 0].max(1))), np.ceil(to_pix(p[..., 0].min(1)))
    r_lo, r_hi = np.floor(to_pix(p[..., 1].max(1))), np.ceil(to_pix(p[..., 1].min(1)))
    return np.stack([np.clip(c_lo, 0, S - 1), np.clip(c_hi, 0, S - 1), np.clip(r_lo, 0, S - 1),
                     np.clip(r_hi, 0, S - 1)], 1).astype(np.int64)


def test_mesh_builders():
    for name, (v, f, c), nv, nf in [("box", rc.box(3, 2, 1), 8, 12), ("tetra", rc.tetra(), 4, 4),
                                    ("octa", rc.octa(), 6, 8)]:
        assert v.shape == (nv, 3) and f.shape == (nf, 3) and c.shape == (nv, 3), name
        assert v.dtype == np.float32 and f.dtype == np.int64 and c.dtype == np.float32
        assert c.min() >= 0 and c.max() <= 1
        p = v.astype(np.float64)[f]
        nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert (np.einsum("fk,fk->f", nrm, p.mean(1)) > 0).all(), name   # outward (convex, centred)
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
        assert (np.unique(e, axis=0, return_counts=True)[1] == 2).all(), name   # closed
    v, f, c = rc.torus(60, 22, 24, 16)
    assert v.shape == (384, 3) and f.shape == (768, 3)
    p = v.astype(np.float64)[f]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    cen = p.mean(1)
    ring = np.concatenate([cen[:, :2] / np.linalg.norm(cen[:, :2], axis=1, keepdims=True) * 60,
                           np.zeros((len(cen), 1))], 1)
    assert (np.einsum("fk,fk->f", nrm, cen - ring) > 0).all()
    (v, f, c), (f1, f2) = rc.double_ellipsoid()
    assert len(f) == 2 * f1 + f2 and (f[:f1] == f[f1 + f2:]).all() and len(v) == len(c)
    for s in range(6):
        q = rc.rotation(s)
        assert np.allclose(q @ q.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(q), 1.0)


@pytest.mark.parametrize("name,seed", ALL)
def test_every_vertex_in_front(name, seed):
    for ndc in rc.ndc64(name, seed):
        assert (ndc[:, 2] > 0).all()
    if name != "double48":   # every other size ends in a partial tile
        assert rc.batch(name, seed)["S"] % rc.TILE != 0


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_s40_properties(seed):
    S = 40
    b = rc.batch("s40", seed)
    assert len({len(m[0]) for m in b["meshes"].values()}) == 5
    assert len({len(m[1]) for m in b["meshes"].values()}) == 5
    # border: centre outside, silhouette across the right and the top border
    _, i, o, ndc = _image("s40", seed, "border")
    u = b["K"][i, 0, 0] * b["t"][i, 0] / b["t"][i, 2] + b["K"][i, 0, 2]
    assert u > S - 1
    cov = _cover(o)
    assert 0.05 <= cov.mean() <= 0.60
    for line in (cov[:, S - 1], cov[0, :]):
        assert line.any() and not line.all()
    assert not cov[:, 0].any() and not cov[S - 1, :].any()
    # closeup: every pixel covered, every tile bins many faces
    _, i, o, ndc = _image("s40", seed, "closeup")
    assert _cover(o).all()
    bb = _pixel_bbox(ndc, b["meshes"][i][1], S)
    for ty in range(0, S, rc.TILE):
        for tx in range(0, S, rc.TILE):
            n = ((bb[:, 1] >= tx) & (bb[:, 0] < tx + rc.TILE) & (bb[:, 3] >= ty) & (bb[:, 2] < ty + rc.TILE)).sum()
            assert n >= 10, (tx, ty, n)
    # bigbox: ≥ 95 % covered, each face's screen bbox spans more than one tile
    _, i, o, ndc = _image("s40", seed, "bigbox")
    assert _cover(o).mean() >= 0.95
    bb = _pixel_bbox(ndc, b["meshes"][i][1], S)
    assert len(bb) == 12
    assert (((bb[:, 1] // rc.TILE) > (bb[:, 0] // rc.TILE)) | ((bb[:, 3] // rc.TILE) > (bb[:, 2] // rc.TILE))).all()
    # needle: slivers, a little coverage
    _, i, o, ndc = _image("s40", seed, "needle")
    assert 0 < _cover(o).mean() < 0.05
    # offscreen: nothing
    _, i, o, ndc = _image("s40", seed, "offscreen")
    assert not _cover(o).any()
    assert (o["zbuf"] == -1).all() and (o["bary"] == -1).all() and (o["images"][..., 3] == 0).all()
    assert (o["images"][..., :3] == 0.5).all()


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_s24_properties(seed):
    b = rc.batch("s24", seed)
    nv = [len(b["meshes"][i][0]) for i in range(7)]
    assert nv[:6] == [8, 4, 42, 8, 6, 8]
    vert_img = np.repeat(np.arange(7), nv)
    assert len(set(vert_img[:64].tolist())) >= 5           # five images in the first wave
    zmin = np.array([n[:, 2].min() for n in rc.ndc64("s24", seed)])
    assert zmin[3] < 400 and (np.delete(zmin, 3) > 400).all()
    sep = rc.lights64("s24", seed, (True, True))
    assert (sep[3] == 0).all() and all(np.abs(sep[i]).max() > 0 for i in range(7) if i != 3)
    assert int(zmin.argmin()) == 3                          # batch minimum: neither first nor last
    assert int(b["t"][:, 2].argmax()) == 6 and int(b["t"][:6, 2].argmax()) == 5
    orc = rc.oracle("s24", seed)
    for i in range(6):
        assert _cover(orc[i]).sum() >= 10, b["names"][i]
    # far: inside a 3×3 pixel block, hundreds of faces per pixel
    cov = _cover(orc[6])
    r, c = np.nonzero(cov)
    assert len(r) > 0 and r.max() - r.min() <= 2 and c.max() - c.min() <= 2
    assert len(b["meshes"][6][1]) / len(r) >= 30 and len(b["meshes"][6][1]) >= 200


def _inside_count(ndc, faces, S):
    """[S, S] number of faces whose fp64 barycentrics are all > 0 at the pixel centre."""
    rr, cc = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    cnt = np.zeros((S, S), np.int64)
    for f in range(len(faces)):
        bary, pz, nd = rc.eval_faces(ndc, faces, np.full(S * S, f), rr.ravel(), cc.ravel(), S)
        cnt += ((bary.min(1) > 0) & (pz >= 0) & nd).reshape(S, S)
    return cnt


def test_torus_properties():
    holes = []
    for seed in rc.SEEDS:
        b, i, o, ndc = _image("torus56", seed, "torus")
        cov = _cover(o)
        assert 0.05 < cov.mean() < 0.9
        cnt = _inside_count(ndc, b["meshes"][0][1], 56)
        assert (cnt >= 4).any()                             # a ray through the tube twice
        ccov = np.cumsum(cov, 1)
        rcov = np.cumsum(cov, 0)
        left, right = ccov > 0, (ccov[:, -1:] - ccov) > 0
        up, down = rcov > 0, (rcov[-1:, :] - rcov) > 0
        holes.append(int((~cov & left & right & up & down).sum()))
    assert max(holes) > 0, holes                            # background inside the hole


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_double_ellipsoid_properties(seed):
    b, i, o, ndc = _image("double48", seed, "double")
    _, (f1, f2) = rc.double_ellipsoid()
    faces = b["meshes"][0][1]
    p = o["p2f"]
    assert (p < f1 + f2).all()                              # the oracle itself: ties → lower index
    first = (p >= 0) & (p < f1)
    assert first.sum() > 50 and ((p >= f1) & (p < f1 + f2)).sum() > 50   # both surfaces visible
    r, c = np.nonzero(first)
    _, pz_a, _ = rc.eval_faces(ndc, faces, p[r, c], r, c, 48)
    _, pz_b, _ = rc.eval_faces(ndc, faces, p[r, c] + f1 + f2, r, c, 48)
    assert (pz_a == pz_b).all()                             # exact ties against a higher index


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_chunks72_properties(seed):
    b, i, o, ndc = _image("chunks72", seed, "chunks")
    assert len(b["meshes"][0][1]) == 1728 and -(-1728 // 256) == 7
    cov = _cover(o)
    assert cov[:, 0].any() and not cov[:, 0].all()          # across the left border
    assert np.unique(o["p2f"][cov] // 256).size >= 3        # winners from several chunks
    assert (o["p2f"] >= 6 * 256).sum() >= 10                # and from the last, partial one


@pytest.mark.parametrize("name,seed", ALL)
def test_float32_oracle_meets_the_rule(name, seed):
    b = rc.batch(name, seed)
    for light in (rc.LIGHTS if name in ("s40", "s24") else rc.LIGHTS[:1]):
        got = rc.oracle(name, seed, light, fp32=True)
        rc.compare_batch(f"fp32-oracle {name} seed {seed} light {light}", got,
                         rc.oracle(name, seed, light), rc.ndc64(name, seed), b["meshes"],
                         b["labels"], b["S"], cap_fraction=0.25, names=b["names"])
    if name == "double48":
        _, (f1, f2) = rc.double_ellipsoid()
        assert (got[0]["p2f"] < f1 + f2).all()


def test_rule_rejects_wrong_faces():
    """The rule itself: a shifted image, a lost tile row and a face from behind the winner are
    not explained away."""
    name, seed = "chunks72", 0
    b = rc.batch(name, seed)
    o = rc.oracle(name, seed)[0]
    ndc, faces, S = rc.ndc64(name, seed)[0], b["meshes"][0][1], b["S"]
    assert rc.compare_with_oracle(o, o, ndc, faces, S)["mismatch"] == 0
    shifted = {k: np.roll(v, 1, axis=1) for k, v in o.items()}          # one pixel to the right
    assert rc.compare_with_oracle(shifted, o, ndc, faces, S)["unexplained"] > 0
    dropped = {k: v.copy() for k, v in o.items()}                        # one tile row lost
    dropped["p2f"][64:] = -1
    dropped["zbuf"][64:] = -1
    assert rc.compare_with_oracle(dropped, o, ndc, faces, S)["unexplained"] > 0
    hidden = {k: v.copy() for k, v in o.items()}                         # a face behind the winner
    r, c = np.nonzero(o["p2f"] >= 0)
    cnt = 0
    for rr, cc in zip(r[::7], c[::7]):
        bary, pz, nd = rc.eval_faces(ndc, faces, np.arange(len(faces)), np.full(len(faces), rr),
                                     np.full(len(faces), cc), S)
        back = np.nonzero((bary.min(1) > 0.05) & nd & (pz > o["zbuf"][rr, cc] * 1.01))[0]
        if len(back):
            hidden["p2f"][rr, cc] = back[0]
            cnt += 1
    assert cnt > 0
    st = rc.compare_with_oracle(hidden, o, ndc, faces, S)
    assert st["unexplained"] >= 1


# ------------------------------------------------------------- the scenes catch a broken kernel
def _restated(name, seed, fault=None, light=(True, True)):
    from tests import render_restatement as rr
    b = rc.batch(name, seed)
    out, lights = rr.render_batch(b, fault, light)
    return b, out, lights


def _check(name, seed, out):
    b = rc.batch(name, seed)
    got = rc.split_batch(out, b["face_offset"])
    return rc.compare_batch(f"restated {name} seed {seed}", got, rc.oracle(name, seed),
                            rc.ndc64(name, seed), b["meshes"], b["labels"], b["S"], names=b["names"])


@pytest.mark.parametrize("name,seed", ALL)
def test_restated_kernel_meets_the_rule(name, seed):
    """The float32 restatement of the kernel's structure (bboxes, tiles, chunks, key minimum),
    unbroken: the rule, the cap, the tie rule and the lights."""
    b, out, lights = _restated(name, seed)
    _check(name, seed, out)
    if name == "double48":
        _, (f1, f2) = rc.double_ellipsoid()
        assert (out["p2f"] < f1 + f2).all()
    for light in rc.LIGHTS:
        np.testing.assert_allclose(_restated(name, seed, None, light)[2] if light != (True, True) else lights,
                                   rc.lights64(name, seed, light), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("fault,name", [("no_partial_tiles", "s40"), ("no_partial_tiles", "s24"),
                                        ("clamp_short", "s40"), ("clamp_short", "chunks72"),
                                        ("drop_last_chunk", "chunks72"), ("drop_last_chunk", "s40"),
                                        ("range_leak", "s24"), ("range_leak", "s40")])
@pytest.mark.parametrize("seed", rc.SEEDS)
def test_scenes_catch_a_broken_rasteriser(fault, name, seed):
    """Each structural fault leaves unexplained pixels (or faces of another image) on the scene
    built for it, with both seeds: test_render_edge_scenes would fail on such a kernel."""
    _, out, _ = _restated(name, seed, fault)
    with pytest.raises(AssertionError):
        _check(name, seed, out)


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_double_ellipsoid_catches_ties_to_the_higher_index(seed):
    """Ties resolved upwards leave no unexplained pixel (an exact tie is a near-tie): the cap on
    explained pixels and the repeated-block assertion catch them."""
    _, out, _ = _restated("double48", seed, "ties_high")
    with pytest.raises(AssertionError, match="restated double48"):
        _check("double48", seed, out)
    _, (f1, f2) = rc.double_ellipsoid()
    assert (out["p2f"] >= f1 + f2).sum() > 50


@pytest.mark.parametrize("seed", rc.SEEDS)
@pytest.mark.parametrize("light", [(True, True), (False, False)])
def test_s24_catches_a_wave_that_reduces_one_image(seed, light):
    """A per-wave minimum that handles only the wave's first image moves the per-image lights and
    the batch-znear light (its minimum is the fourth image of the first wave)."""
    _, _, lights = _restated("s24", seed, "zmin_first_image", light)
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(lights, rc.lights64("s24", seed, light), rtol=1e-5, atol=1e-3)
