"""GPU: UV-textured meshes on the HIP renderer (``scflow_render_textured``) against the fp64
restatement of pytorch3d's texture sampling and Phong shading (tests/render_uv_restatement.py;
parity with pytorch3d itself is UNPINNED, it is absent), evaluated at the kernel's own fragments
so that sampling is judged apart from rasterisation, which tests/test_gpu_render.py judges.

Sampling tolerance, derived: 16·2⁻²³·max(H, W) absolute on covered pixels — the interpolated uv
and its scaling by (W − 1) lose a few ulps of a value ≤ 1, the tap weights inherit that times the
map size, the contrast between neighbouring texels is ≤ 1; both axes and a factor 2 of margin.
Observed maxima per map size: DESIGN.md §21.  Full Phong: RGBA 2e-3, the project's image tolerance
(tests/render_cases.py).  Renders are at most 64² except the refiner's, which stays at the 256² of
the other refiner tests."""
import ctypes

import numpy as np
import pytest
import torch

import oracle.render_oracle as ro
from scflow_amd import _lib, synthetic
from scflow_amd.renderer import Renderer, verts_normals
from tests import render_cases as rc
from tests import render_uv_restatement as uvr

pytestmark = pytest.mark.gpu

DEV = "cuda"


def sampling_tol(h, w):
    return 16.0 * 2.0 ** -23 * max(h, w)


# ------------------------------------------------------------------------ through the C ABI
class Packed:
    """A list of mesh dicts packed for ``scflow_render`` / ``scflow_render_textured`` the way
    ``Renderer.forward`` packs them, with every array the caller may want to break."""

    def __init__(self, meshes, R, t, K, S, colours=(1.0, 0.0, 0.0)):
        n = self.n = len(meshes)
        self.S, self.meshes = S, meshes
        nv, nf = [len(m["verts"]) for m in meshes], [len(m["faces"]) for m in meshes]
        voff = np.concatenate([[0], np.cumsum(nv)[:-1]])
        self.face_offset = np.concatenate([[0], np.cumsum(nf)])
        T = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)  # noqa: E731
        self.verts = T(np.concatenate([m["verts"] for m in meshes]))
        self.colors = T(np.concatenate([m["colors"] for m in meshes]))
        self.normals = torch.cat([verts_normals(torch.from_numpy(m["verts"]).double(),
                                                torch.from_numpy(m["faces"])).float() for m in meshes]).to(DEV)
        self.faces = T(np.concatenate([m["faces"] + o for m, o in zip(meshes, voff)]), torch.int32)
        self.vert_img = T(np.repeat(np.arange(n), nv), torch.int32)
        self.face_img = T(np.repeat(np.arange(n), nf), torch.int32)
        self.R, self.t, self.K = T(R), T(t), T(K)
        amb, dif, spe = colours
        self.params = torch.tensor([amb] * 3 + [dif] * 3 + [spe] * 3 + [0.5] * 3 + [0.0, 1.0, 0.0], device=DEV)
        self.ws = torch.zeros(int(_lib.load().scflow_render_workspace(n, S, self.verts.shape[0])),
                              dtype=torch.uint8, device=DEV)
        # textures: RGBA8 maps back to back, host tables, packed uvs
        self.tex_offset = np.full(n, -1, np.int64)
        self.tex_hw = np.zeros((n, 2), np.int32)
        maps, uvs, fuvs, pos, nuv = [], [], [], 0, 0
        for i, m in enumerate(meshes):
            if m.get("texture") is None:
                fuvs.append(np.zeros((nf[i], 3), np.int64))
                continue
            h, w = m["texture"].shape[:2]
            maps.append(np.concatenate([m["texture"], np.full((h, w, 1), 255, np.uint8)], 2).reshape(-1))
            self.tex_offset[i], self.tex_hw[i] = pos, (h, w)
            pos += h * w * 4
            uvs.append(m["verts_uvs"])
            fuvs.append(m["faces_uvs"] + nuv)
            nuv += len(m["verts_uvs"])
        self.total_uvs = nuv
        self.texels = T(np.concatenate(maps) if maps else np.zeros(4, np.uint8), torch.uint8)
        self.verts_uvs = T(np.concatenate(uvs) if uvs else np.zeros((1, 2), np.float32))
        self.faces_uvs = T(np.concatenate(fuvs), torch.int32)

    def outputs(self, fill=None):
        n, S = self.n, self.S
        mk = (lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=DEV)) if fill is None else \
            (lambda *s, dt=torch.float32: torch.full(s, fill, dtype=dt, device=DEV))
        return dict(images=mk(n, S, S, 4), zbuf=mk(n, S, S), p2f=mk(n, S, S, dt=torch.int32),
                    bary=mk(n, S, S, 3), light=mk(n, 3))

    def args(self, out):
        a = _lib.RenderArgs()
        a.verts, a.normals, a.colors, a.faces = (self.verts.data_ptr(), self.normals.data_ptr(),
                                                 self.colors.data_ptr(), self.faces.data_ptr())
        a.vert_img, a.face_img = self.vert_img.data_ptr(), self.face_img.data_ptr()
        a.R, a.t, a.K = self.R.data_ptr(), self.t.data_ptr(), self.K.data_ptr()
        a.n_img, a.size, a.total_verts, a.total_faces = self.n, self.S, self.verts.shape[0], self.faces.shape[0]
        a.light_mode = _lib.SCFLOW_LIGHT_PER_IMAGE
        base = self.params.data_ptr()
        a.ambient, a.diffuse, a.specular, a.background = base, base + 12, base + 24, base + 36
        a.light_location = base + 48
        a.shininess = 64.0
        a.images, a.zbuf, a.pix_to_face, a.bary = (out["images"].data_ptr(), out["zbuf"].data_ptr(),
                                                   out["p2f"].data_ptr(), out["bary"].data_ptr())
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws.numel()
        a.light_out = out["light"].data_ptr()
        return a

    def tex(self, **over):
        x = _lib.RenderTex()
        x.texels, x.texel_bytes = self.texels.data_ptr(), self.texels.numel()
        x.tex_offset, x.tex_hw = self.tex_offset.ctypes.data, self.tex_hw.ctypes.data
        x.verts_uvs, x.faces_uvs, x.total_uvs = self.verts_uvs.data_ptr(), self.faces_uvs.data_ptr(), self.total_uvs
        for k, v in over.items():
            setattr(x, k, v)
        return x

    def render(self, how="textured"):
        """how: 'textured' (scflow_render_textured with the maps), 'null' (tex = NULL), 'plain'
        (scflow_render).  Returns the outputs as numpy arrays."""
        lib, out = _lib.load(), self.outputs()
        a, stream = self.args(out), torch.cuda.current_stream().cuda_stream
        if how == "plain":
            code = lib.scflow_render(ctypes.byref(a), stream)
        else:
            x = self.tex()
            code = lib.scflow_render_textured(ctypes.byref(a), ctypes.byref(x) if how == "textured" else None, stream)
        assert code == 0, (how, code)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}


_SCENES = {}


def _sampling(S):
    """The sampling scene at S, rendered once: (scene, Packed, textured / null / plain outputs)."""
    if S not in _SCENES:
        sc = uvr.sampling_scene(S)
        p = Packed(sc["meshes"], sc["R"], sc["t"], sc["K"], S)
        _SCENES[S] = (sc, p, p.render("textured"), p.render("null"), p.render("plain"))
    return _SCENES[S]


def _texel_diffs(meshes, face_offset, out, only_faces=None):
    """Per image: max |kernel RGB − restated texel| over the covered pixels (of ``only_faces``),
    at the kernel's own pix_to_face and barycentrics; ambient 1, diffuse 0, specular 0."""
    diffs = []
    for i, m in enumerate(meshes):
        p = out["p2f"][i].astype(np.int64)
        local = np.where(p >= 0, p - int(face_offset[i]), -1)
        want = uvr.texel_image(m, local, out["bary"][i]).numpy()
        hit = local >= 0
        if only_faces is not None:
            hit &= np.isin(local, only_faces)
        d = np.abs(out["images"][i][..., :3].astype(np.float64) - want)[hit]
        diffs.append((int(hit.sum()), float(d.max()) if d.size else 0.0))
    return diffs


@pytest.mark.parametrize("S", [24, 40])
def test_sampling_matches_restatement_at_the_kernels_fragments(S):
    sc, p, out, _, _ = _sampling(S)
    diffs = _texel_diffs(sc["meshes"], p.face_offset, out)
    worst = {}
    for tag, m, (cnt, d) in zip(sc["tags"], sc["meshes"], diffs):
        hw = m["texture"].shape[:2]
        worst[hw] = max(worst.get(hw, 0.0), d)
        print(f"S={S} {tag}: {cnt} covered pixels, max |rgb - texel| {d:.3e} (tolerance {sampling_tol(*hw):.3e})")
    print("S=%d largest difference per map size: %s" % (S, {f"{h}x{w}": f"{d:.2e}" for (h, w), d in worst.items()}))
    for i, (tag, m, (cnt, d)) in enumerate(zip(sc["tags"], sc["meshes"], diffs)):
        assert cnt >= 0.1 * S * S, (tag, cnt)
        assert d <= sampling_tol(*m["texture"].shape[:2]), (tag, d)
        bg = out["p2f"][i] < 0
        assert bg.any() and (out["images"][i][bg] == np.array([0.5, 0.5, 0.5, 0.0], np.float32)).all(), tag
        assert (out["images"][i][~bg][:, 3] == 1.0).all(), tag
    # the scene does exercise what it claims: clamped uvs, and both sides of the seam
    wide = [i for i, t in enumerate(sc["tags"]) if t.endswith("-wide")]
    uv = uvr.pixel_uvs(sc["meshes"][wide[0]], np.where(out["p2f"][wide[0]] >= 0, out["p2f"][wide[0]] -
                                                       p.face_offset[wide[0]], -1), out["bary"][wide[0]]).numpy()
    assert uv.min() < -0.1 and uv.max() > 1.1


@pytest.mark.parametrize("S", [24, 40])
def test_geometry_and_untextured_path_are_untouched(S):
    _, p, tex, null, plain = _sampling(S)
    for k in ("zbuf", "p2f", "bary", "light"):
        assert np.array_equal(tex[k], plain[k]), k
        assert np.array_equal(null[k], plain[k]), k
    assert np.array_equal(null["images"], plain["images"])       # tex = NULL: scflow_render's bits
    assert np.array_equal(tex["images"][..., 3], plain["images"][..., 3])
    assert not np.array_equal(tex["images"], plain["images"])


def test_more_images_than_one_shading_launch_holds():
    """The texture table travels 64 images per shading launch: 80 images (the sampling scene four
    times over, every third image vertex-coloured) put maps on both sides of that boundary."""
    S = 24
    sc = uvr.sampling_scene(S)
    sel = [i % 20 for i in range(80)]
    ms = [sc["meshes"][i] if k % 3 else dict(sc["meshes"][i], texture=None) for k, i in enumerate(sel)]
    p = Packed(ms, sc["R"][sel], sc["t"][sel], sc["K"][sel], S)
    assert (p.tex_offset[:64] >= 0).any() and (p.tex_offset[64:] >= 0).any() and (p.tex_offset[64:] < 0).any()
    out, plain = p.render("textured"), p.render("plain")
    for k in ("zbuf", "p2f", "bary", "light"):
        assert np.array_equal(out[k], plain[k]), k
    tex = [k for k in range(80) if k % 3]
    flat = [k for k in range(80) if not k % 3]
    assert np.array_equal(out["images"][flat], plain["images"][flat])
    d = _texel_diffs([ms[k] for k in tex], p.face_offset[tex], {k: v[tex] for k, v in out.items() if k != "light"})
    for k, (cnt, diff) in zip(tex, d):
        assert cnt > 0 and diff <= sampling_tol(*ms[k]["texture"].shape[:2]), (k, sc["tags"][sel[k]], diff)


# ------------------------------------------------------------------------ through Renderer
def _phong_batch(S=64):
    """Three textured ellipsoids (maps 16×16, 7×64, 5×4) and a vertex-coloured one, posed like the
    images of tests/render_cases.py."""
    meshes, R, t, K = {}, [], [], []
    for i, hw in enumerate([(16, 16), (7, 64), (5, 4), None]):
        semi = np.array([60.0, 46.0, 36.0]) * (1.0 + 0.1 * i)
        if hw is None:
            v, f, c = synthetic.ellipsoid_mesh(semi, 10, 14)
            meshes[i] = dict(verts=v, faces=f, colors=c)
        else:
            meshes[i] = synthetic.textured_ellipsoid_mesh(semi, 8 + 2 * i, 12 + 4 * i, hw, seed=i)
        R.append(rc.rotation(60 + i) if i else uvr.SEAM_R)
        tz = 600.0 + 90.0 * i
        t.append([5.0 * i - 8.0, 6.0 - 4.0 * i, tz])
        f = S * tz / (2.6 * semi[0])
        K.append([[f, 0, (S - 1) / 2 + 0.4 * i], [0, 1.05 * f, (S - 1) / 2 - 0.3 * i], [0, 0, 1]])
    return dict(S=S, meshes=meshes, R=np.stack(R).astype(np.float32), t=np.array(t, np.float32),
                K=np.array(K, np.float32), labels=np.arange(4, dtype=np.int64))


def _renderer(b, light=(True, True), labels=None, **kw):
    labels = list(b["meshes"]) if labels is None else labels
    return Renderer(image_size=(b["S"], b["S"]), soft_blending=False, render_mask=False,
                    seperate_lights=light[0], default_lights=light[1],
                    meshes={lab: b["meshes"][lab] for lab in labels}, **kw)


def _run(r, b, idx):
    out = r(*(torch.from_numpy(np.ascontiguousarray(b[k][idx])).to(DEV) for k in ("R", "t", "K", "labels")))
    torch.cuda.synchronize()
    fr = out["fragments"]
    return dict(p2f=fr.pix_to_face[..., 0].cpu().numpy(), zbuf=fr.zbuf[..., 0].cpu().numpy(),
                bary=fr.bary_coords[..., 0, :].cpu().numpy(), images=out["images"].cpu().numpy(),
                light=out["light_location"].cpu().numpy())


def _assert_phong(tag, b, idx, got, light):
    """Images against the restatement at the kernel's fragments (RGBA 2e-3)."""
    off = np.concatenate([[0], np.cumsum([len(b["meshes"][int(b["labels"][i])]["faces"]) for i in idx])])
    per = rc.split_batch(dict(p2f=got["p2f"], zbuf=got["zbuf"], bary=got["bary"], images=got["images"]), off)
    T = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
    lights = ro.light_location([T(b["meshes"][int(b["labels"][i])]["verts"]) for i in idx],
                               T(b["R"][idx]), T(b["t"][idx]), light).numpy()
    np.testing.assert_allclose(got["light"], lights, rtol=1e-5, atol=1e-3)
    for k, i in enumerate(idx):
        m = b["meshes"][int(b["labels"][i])]
        want = uvr.shade_image(m, per[k]["p2f"], per[k]["bary"], b["R"][i], b["t"][i], lights[k],
                               **uvr.LIGHT_COLOURS[light[1]]).numpy()
        d = np.abs(per[k]["images"].astype(np.float64) - want)
        hit = per[k]["p2f"] >= 0
        print(f"{tag}[{i}]: {int(hit.sum())} covered, max |rgba - restatement| {d[hit].max():.3e}")
        assert hit.sum() > 200 and d[hit].max() <= rc.RGB_ATOL, (tag, i, d[hit].max())
        assert (per[k]["images"][~hit] == np.array([0.5, 0.5, 0.5, 0.0], np.float32)).all(), (tag, i)
    return per


@pytest.mark.parametrize("light", rc.LIGHTS, ids=[f"sep{int(s)}def{int(d)}" for s, d in rc.LIGHTS])
def test_full_phong_through_renderer(light):
    b = _phong_batch()
    idx = [0, 1, 2, 3]
    got = _run(_renderer(b, light).to(DEV), b, idx)
    per = _assert_phong(f"phong {light}", b, idx, got, light)
    # the fragments against the fp64 oracle, under the per-pixel rule of tests/render_cases.py
    tuples = {lab: (m["verts"], m["faces"], m["colors"]) for lab, m in b["meshes"].items()}
    orc = rc.run_oracle(tuples, b["R"], b["t"], b["K"], b["labels"], b["S"], light)
    for o in orc:
        o.pop("images")     # the oracle shades vertex colours
    frags = [dict(p2f=p["p2f"], zbuf=p["zbuf"], bary=p["bary"]) for p in per]
    ndcs = [rc.project64(tuples[i][0], b["R"][i], b["t"][i], b["K"][i], b["S"]) for i in idx]
    rc.compare_batch(f"uv fragments {light}", frags, orc, ndcs, tuples, b["labels"], b["S"])


def test_seam_needs_per_corner_uvs():
    """Pixels of the faces that touch the seam column match the restatement within the sampling
    tolerance; with the seam's corners given the shared vertex's single uv (what per-vertex
    colours or per-vertex uvs can express) they do not: the test can see the seam."""
    S, n_lat, n_lon, hw = 40, 6, 8, (7, 64)
    m = synthetic.textured_ellipsoid_mesh((50.0, 38.0, 30.0), n_lat, n_lon, hw, seed=3)
    sc = uvr.sampling_scene(S)
    i = sc["tags"].index("ell-7x64")
    seam = uvr.seam_faces(n_lat, n_lon)
    pose = (sc["R"][i:i + 1], sc["t"][i:i + 1], sc["K"][i:i + 1], S)
    good = Packed([m], *pose)
    cnt, d = _texel_diffs([m], good.face_offset, good.render(), only_faces=seam)[0]
    print(f"seam: {cnt} pixels on seam faces, max |rgb - texel| {d:.3e}")
    assert cnt >= 30 and d <= sampling_tol(*hw)
    flat = Packed([uvr.per_vertex_uvs(m, n_lat, n_lon)], *pose)
    cnt2, d2 = _texel_diffs([m], flat.face_offset, flat.render(), only_faces=seam)[0]
    print(f"seam, per-vertex emulation: max |rgb - texel| {d2:.3e}")
    assert cnt2 == cnt and d2 > 0.1


def test_mixed_batch_equals_single_images():
    """One batch: a textured mesh twice (one label, one stored map), a vertex-coloured mesh, a
    textured mesh with another map size.  Each image equals its single-image render bit for bit,
    and the vertex-coloured one equals what scflow_render gives."""
    b = _phong_batch()
    idx = [0, 3, 0, 1]
    b = dict(b, R=b["R"][[0, 3, 2, 1]], t=b["t"][[0, 3, 2, 1]], K=b["K"][[0, 3, 2, 1]],
             labels=np.array([0, 3, 0, 1], np.int64))
    r = _renderer(b).to(DEV)
    whole = _run(r, b, [0, 1, 2, 3])
    assert len(r.texture_store()["offset"]) == 3      # labels 0, 1, 2: one map each
    off = np.concatenate([[0], np.cumsum([len(b["meshes"][lab]["faces"]) for lab in idx])])
    for k in range(4):
        one = _run(r, b, [k])
        for key in ("zbuf", "bary", "images", "light"):
            assert np.array_equal(one[key][0], whole[key][k]), (k, key)
        p = whole["p2f"][k]
        assert np.array_equal(one["p2f"][0], np.where(p >= 0, p - off[k], -1)), k
    assert not np.array_equal(whole["images"][0], whole["images"][2])   # same map, another pose
    m = b["meshes"][3]
    plain = Packed([m], b["R"][1:2], b["t"][1:2], b["K"][1:2], b["S"], colours=(0.5, 0.3, 0.2)).render("plain")
    for key, pk in (("zbuf", "zbuf"), ("bary", "bary"), ("images", "images")):
        assert np.array_equal(plain[pk][0], whole[key][1]), key


def test_texel_store_is_built_once_per_device():
    b = _phong_batch(S=24)
    r = _renderer(b, labels=[0, 1])            # built on the CPU
    assert r.texture_store("cpu")["texels"].device.type == "cpu"
    r.to(DEV)
    idx = [0, 1]
    first = _run(r, b, idx)
    store = r.texture_store()["texels"]        # held: its address cannot be handed out again
    assert store.is_cuda and store.numel() == 4 * (16 * 16 + 7 * 64)
    again = _run(r, b, idx)
    assert r.texture_store()["texels"].data_ptr() == store.data_ptr()
    assert np.array_equal(first["images"], again["images"])
    r.add_mesh(2, **b["meshes"][2])
    third = _run(r, b, [0, 1, 2])
    new = r.texture_store()["texels"]
    assert new.data_ptr() != store.data_ptr() and new.numel() == store.numel() + 4 * 5 * 4
    assert np.array_equal(third["images"][:2], first["images"])
    assert (first["p2f"] >= 0).any()


def test_obj_directory_renders_its_texture(tmp_path):
    """``Renderer(mesh_dir=..., mesh_ext='obj')`` on an OBJ + MTL + PNG written to disk: the image
    is the textured one (the restatement's, and the array-fed renderer's bits), not a white object."""
    Image = pytest.importorskip("PIL.Image")
    b = _phong_batch()
    m = b["meshes"][1]
    Image.fromarray(m["texture"], "RGB").save(str(tmp_path / "skin.png"))
    (tmp_path / "m.mtl").write_text("newmtl skin\nKd 1 1 1\nmap_Kd skin.png\n")
    lines = ["mtllib m.mtl", "usemtl skin"]
    lines += ["v %.9g %.9g %.9g" % tuple(v) for v in m["verts"].tolist()]
    lines += ["vt %.9g %.9g" % tuple(v) for v in m["verts_uvs"].tolist()]
    lines += ["f " + " ".join(f"{a + 1}/{t + 1}" for a, t in zip(f, ft))
              for f, ft in zip(m["faces"].tolist(), m["faces_uvs"].tolist())]
    (tmp_path / "obj_000002.obj").write_text("\n".join(lines) + "\n")
    r = Renderer(mesh_dir=str(tmp_path), mesh_ext="obj", image_size=(64, 64), soft_blending=False,
                 render_mask=False, seperate_lights=True).to(DEV)
    assert sorted(r.textures) == [1]
    got = _run(r, b, [1])
    white = dict(m, texture=None, colors=np.ones_like(m["verts"]))
    b1 = dict(b, meshes={1: dict(m, colors=np.ones_like(m["verts"]))})
    _assert_phong("obj directory", b1, [1], got, (True, True))
    hit = got["p2f"][0] >= 0
    flat = uvr.shade_image(white, got["p2f"][0], got["bary"][0], b["R"][1], b["t"][1], got["light"][0]).numpy()
    assert (np.abs(got["images"][0] - flat)[hit][:, :3].max(1) > 0.05).mean() > 0.5
    fed = _run(_renderer(b, labels=[1]).to(DEV), b, [1])
    assert np.array_equal(fed["images"], got["images"])


def test_refiner_renders_textured_meshes():
    """SCFlowRefiner on textured ``meshes=``: ``render`` gives the textured images (they differ
    from the untextured ones and match the restatement), ``refine`` with two cycles runs."""
    from scflow_amd import MODELS
    from tests.test_gpu_decoder import decoder_cfg
    from tests.helpers import refiner_state_dict
    S, B = 256, 2   # not ≤ 64: the decoder's kernels are tiled for 256², as in the other refiner tests
    sc = synthetic.make_scene(B, S, seed=21)
    labs = sorted(set(sc["labels"].tolist()))
    meshes = {}
    for k, lab in enumerate(labs):
        semi = np.array(synthetic.ELLIPSOID_AXES) * synthetic.YCBV_DIAMETERS[lab]
        meshes[lab] = synthetic.textured_ellipsoid_mesh(semi, 12, 24, [(16, 16), (7, 64)][k % 2], seed=k)
    enc = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic", norm_cfg=dict(type="IN"))
    ctx = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic", norm_cfg=dict(type="BN"))

    def build(ms):
        r = MODELS.build(dict(type="SCFlowRefiner", cxt_channels=128, h_channels=128, seperate_encoder=False,
                              encoder=enc, cxt_encoder=ctx, decoder=dict(type="SCFlowDecoder", **decoder_cfg(2)),
                              renderer=dict(mesh_dir=None, image_size=(S, S), soft_blending=False,
                                            render_mask=False, seperate_lights=True, meshes=ms),
                              test_cfg=dict(iters=2, cycles=2)))
        r.load_state_dict({("decoder." + k if not k.startswith(("real_encoder.", "render_encoder.", "context."))
                            else k): v for k, v in refiner_state_dict().items()}, strict=False)
        return r.eval().cuda()
    r = build(meshes)
    R, t, K, lab = (torch.from_numpy(sc[k]).cuda() for k in ("ref_rotation", "ref_translation",
                                                             "internel_k", "labels"))
    img, depth, mask = r.render(R, t, K, lab)
    plain = Renderer(image_size=(S, S), soft_blending=False, render_mask=False, seperate_lights=True,
                     meshes={l: (m["verts"], m["faces"], m["colors"]) for l, m in meshes.items()}).to(DEV)
    flat = plain(R, t, K, lab)
    assert torch.equal(depth, flat["fragments"].zbuf[..., 0])
    cov = mask > 0
    assert cov.sum() > 1000
    assert ((img - flat["images"][..., :3].permute(0, 3, 1, 2)).abs().amax(1)[cov] > 0.05).float().mean() > 0.5
    b = dict(S=S, meshes=meshes, R=sc["ref_rotation"], t=sc["ref_translation"], K=sc["internel_k"],
             labels=sc["labels"].astype(np.int64))
    direct = r.renderer(R, t, K, lab)
    torch.testing.assert_close(img, direct["images"][..., :3].permute(0, 3, 1, 2))
    fr = direct["fragments"]
    got = dict(p2f=fr.pix_to_face[..., 0].cpu().numpy(), zbuf=fr.zbuf[..., 0].cpu().numpy(),
               bary=fr.bary_coords[..., 0, :].cpu().numpy(), images=direct["images"].cpu().numpy(),
               light=direct["light_location"].cpu().numpy())
    _assert_phong("refiner", b, list(range(B)), got, (True, True))
    tgt = synthetic.make_train_targets(sc, S, seed=21)
    real, _, _ = r.render(torch.from_numpy(tgt["gt_rotation"]).cuda(),
                          torch.from_numpy(tgt["gt_translation"]).cuda(), K, lab)
    R2, t2, _ = r.refine(real, R, t, K, lab, cycles=2)
    torch.cuda.synchronize()
    assert torch.isfinite(R2).all() and torch.isfinite(t2).all()


# ------------------------------------------------------------------------ argument errors
def test_render_textured_rejects_bad_arguments():
    """Every SCFLOW_EINVAL case of scflow_render_textured: non-zero, and nothing written (every
    device pointer stays valid, every buffer keeps its fill)."""
    lib = _lib.load()
    sc = uvr.sampling_scene(24)
    keep = [sc["tags"].index(t) for t in ("quad-2x3", "ell-5x4")]
    ms = [sc["meshes"][keep[0]], dict(sc["meshes"][keep[1]], texture=None), sc["meshes"][keep[1]]]
    sel = [keep[0], keep[1], keep[1]]
    p = Packed(ms, sc["R"][sel], sc["t"][sel], sc["K"][sel], 24)
    assert p.tex_offset.tolist() == [0, -1, 24]
    sentinel = 777.0
    out = p.outputs(fill=sentinel)
    stream = torch.cuda.current_stream().cuda_stream
    hw0, hw1, odd, far = p.tex_hw.copy(), p.tex_hw.copy(), p.tex_offset.copy(), p.tex_offset.copy()
    hw0[0, 0], hw1[2, 1] = 0, -3
    odd[2] += 2
    far[2] = p.texels.numel() - 4 * 5 * 4 + 4
    cases = [dict(texels=None), dict(tex_offset=None), dict(tex_hw=None), dict(verts_uvs=None),
             dict(faces_uvs=None), dict(total_uvs=0), dict(total_uvs=-5),
             dict(tex_hw=hw0.ctypes.data), dict(tex_hw=hw1.ctypes.data),
             dict(tex_offset=odd.ctypes.data), dict(tex_offset=far.ctypes.data),
             dict(texel_bytes=p.texels.numel() - 1)]
    for over in cases:
        a, x = p.args(out), p.tex(**over)
        assert lib.scflow_render_textured(ctypes.byref(a), ctypes.byref(x), stream) == -1, over
        torch.cuda.synchronize()
        for k, v in out.items():
            assert (v == (777 if k == "p2f" else sentinel)).all(), (over, k)
        assert (p.ws == 0).all(), over
    a = p.args(out)
    a.n_img = 0       # scflow_render's own checks come first
    assert lib.scflow_render_textured(ctypes.byref(a), ctypes.byref(p.tex()), stream) == -1
    # every image untextured: the arrays the textured images would need may be NULL
    none = np.full(3, -1, np.int64)
    a, x = p.args(out), p.tex(tex_offset=none.ctypes.data, texels=None, tex_hw=None, verts_uvs=None,
                              faces_uvs=None, total_uvs=0)
    assert lib.scflow_render_textured(ctypes.byref(a), ctypes.byref(x), stream) == 0
    torch.cuda.synchronize()
    flat = {k: v.cpu().numpy() for k, v in out.items()}
    plain = p.render("plain")
    for k in plain:
        assert np.array_equal(flat[k], plain[k]), k
    # and the unbroken arguments render; the untextured image in the middle is scflow_render's
    full = p.render("textured")
    assert np.array_equal(full["images"][1], plain["images"][1])
    assert not np.array_equal(full["images"][2], plain["images"][2])
    d = _texel_diffs([ms[0], ms[2]], p.face_offset[[0, 2]],
                     {k: v[[0, 2]] for k, v in full.items() if k != "light"})
    assert max(x[1] for x in d) <= sampling_tol(5, 4)
