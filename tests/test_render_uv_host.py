"""CPU: UV-textured meshes up to the device boundary — the OBJ / MTL / image readers, ``add_mesh``'s
validation, the mesh registry, the test-side restatement of pytorch3d's texture sampling
(tests/render_uv_restatement.py) pinned to a closed form, and the new C-ABI struct."""
import ctypes
import os

import numpy as np
import pytest
import torch

from scflow_amd import _lib, renderer, synthetic
from scflow_amd.renderer import Renderer, load_obj, load_obj_textured
from tests import render_uv_restatement as uvr
from tests.test_abi import test_struct_layout_matches_header as _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a unit square and an apex: 5 vertices, 6 texture coordinates (vertex 1 has two: a seam)
V = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 0.5 1\n"
VT = "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvt 0.5 0.5\nvt 0.25 0.75\n"
MTL = "newmtl plain\nKd 0.8 0.8 0.8\n\nnewmtl skin\nKd 1 1 1\nmap_Kd -s 1 1 1 maps/skin.png\n"


def _png(path, arr, mode):
    Image = pytest.importorskip("PIL.Image")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr, mode).save(path)


def _write(tmp_path, body, mtl=MTL, name="obj_000003.obj"):
    p = tmp_path / name
    p.write_text(("mtllib mesh.mtl\n" if mtl else "") + body)
    if mtl:
        (tmp_path / "mesh.mtl").write_text(mtl)
    return str(p)


def _rgb(h=3, w=4):
    return np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------ OBJ reader
def test_obj_corner_forms_polygons_and_negative_indices(tmp_path):
    pytest.importorskip("PIL")
    img = _rgb()
    _png(str(tmp_path / "maps" / "skin.png"), img, "RGB")
    body = (V + VT + "vn 0 0 1\nusemtl skin\n"
            "f 1/1 2/2 3/3 4/4\n"              # a quad, v/vt
            "f 1/1/1 2/6/1 5/5/1\n"            # v/vt/vn; vertex 2 with its second coordinate
            "f -5/-6 -4/-5 -3/-4 -2/-3 -1/-2\n")  # a pentagon, relative indices
    m = load_obj_textured(_write(tmp_path, body))
    assert m["verts"].shape == (5, 3) and m["verts"].dtype == np.float32
    assert m["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    assert m["faces_uvs"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 5, 4], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    assert m["faces"].dtype == m["faces_uvs"].dtype == np.int64
    np.testing.assert_array_equal(m["verts_uvs"], np.array([[0, 0], [1, 0], [1, 1], [0, 1], [.5, .5],
                                                            [.25, .75]], np.float32))
    # the second material's map (the first has none), relative to the OBJ's directory
    assert m["texture"].dtype == np.uint8 and np.array_equal(m["texture"], img)
    assert m["colors"] is None
    v, f, c = load_obj(_write(tmp_path, body))
    assert np.array_equal(v, m["verts"]) and np.array_equal(f, m["faces"]) and c is None


def test_obj_without_vt_or_without_map_keeps_vertex_colours(tmp_path):
    body = "v 0 0 0 1 0 0\nv 1 0 0 0 1 0\nv 0 1 0 0 0 1\nvn 0 0 1\nf 1//1 2//1 3//1\n"
    for mtl in (MTL, None):          # a map but no vt; neither (no image file is opened)
        m = load_obj_textured(_write(tmp_path, body, mtl))
        assert m["verts_uvs"] is None and m["faces_uvs"] is None and m["texture"] is None
        assert m["faces"].tolist() == [[0, 1, 2]]
        np.testing.assert_array_equal(m["colors"], np.eye(3, dtype=np.float32))
        v, f, c = load_obj(_write(tmp_path, body, mtl))
        assert np.array_equal(v, m["verts"]) and np.array_equal(f, m["faces"]) and np.array_equal(c, m["colors"])
    # vt but no material with a map
    m = load_obj_textured(_write(tmp_path, V + VT + "f 1/1 2/2 3/3\n", "newmtl plain\nKd 1 1 1\n"))
    assert m["verts_uvs"] is None and m["texture"] is None and m["colors"] is None


def test_obj_map_with_a_corner_without_vt_raises(tmp_path):
    os.makedirs(tmp_path / "maps")   # raised before the image is decoded: any bytes do, PIL or not
    (tmp_path / "maps" / "skin.png").write_bytes(b"not decoded")
    p = _write(tmp_path, V + VT + "f 1/1 2/2 3/3\nf 1/1 3 4/4\n")
    with pytest.raises(_lib.ScflowError, match="triangle 1"):
        load_obj_textured(p)
    with pytest.raises(_lib.ScflowError):
        Renderer(mesh_dir=str(tmp_path), mesh_ext="obj", soft_blending=False, render_mask=False)
    assert load_obj(p)[1].tolist() == [[0, 1, 2], [0, 2, 3]]   # the geometry alone still reads


@pytest.mark.parametrize("vt", [False, True])
def test_obj_with_a_dangling_mtllib_loads_untextured(tmp_path, vt):
    """An OBJ that names an MTL file which is not there loaded before textures were read, and
    still does: geometry and vertex colours, no texture; with ``vt`` a warning says why (as
    pytorch3d's), without ``vt`` no MTL is looked for at all."""
    import warnings
    cv = "v 0 0 0 1 0 0\nv 1 0 0 0 1 0\nv 0 1 0 0 0 1\n"
    body = "mtllib gone.mtl\n" + cv + ("vt 0 0\nvt 1 0\nvt 0 1\nf 1/1 2/2 3/3\n" if vt else "f 1 2 3\n")
    p = tmp_path / "obj_000002.obj"
    p.write_text(body)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = load_obj_textured(str(p))
        r = Renderer(mesh_dir=str(tmp_path), mesh_ext="obj", soft_blending=False, render_mask=False)
    assert [("Mtl file does not exist" in str(x.message)) for x in w] == [True] * (2 if vt else 0)
    assert m["verts_uvs"] is None and m["faces_uvs"] is None and m["texture"] is None
    assert m["faces"].tolist() == [[0, 1, 2]]
    np.testing.assert_array_equal(m["colors"], np.eye(3, dtype=np.float32))
    v, f, c = load_obj(str(p))
    assert np.array_equal(v, m["verts"]) and np.array_equal(f, m["faces"]) and np.array_equal(c, m["colors"])
    assert sorted(r.meshes) == [1] and not r.textures
    assert np.array_equal(r.meshes[1][2].numpy(), np.eye(3, dtype=np.float32))


def test_obj_with_a_missing_map_image_loads_untextured(tmp_path):
    """``map_Kd`` names an image that is not there: a warning and no texture, as in pytorch3d
    ("Texture file does not exist"), not an error: such a file loaded before textures were read."""
    p = _write(tmp_path, V + VT + "f 1/1 2/2 3/3\n")   # MTL's maps/skin.png is never written
    with pytest.warns(UserWarning, match="Texture file does not exist"):
        m = load_obj_textured(p)
    assert m["verts_uvs"] is None and m["texture"] is None and m["faces"].tolist() == [[0, 1, 2]]
    with pytest.warns(UserWarning, match="Texture file does not exist"):
        r = Renderer(mesh_dir=str(tmp_path), mesh_ext="obj", soft_blending=False, render_mask=False)
    assert sorted(r.meshes) == [2] and not r.textures


def test_mtllib_name_with_spaces_and_several_names(tmp_path):
    pytest.importorskip("PIL")
    img = _rgb()
    _png(str(tmp_path / "maps" / "skin.png"), img, "RGB")
    body = V + VT + "f 1/1 2/2 3/3\n"
    (tmp_path / "my mesh.mtl").write_text(MTL)
    (tmp_path / "a.obj").write_text("mtllib my mesh.mtl\n" + body)     # one name with a space
    (tmp_path / "mesh.mtl").write_text(MTL)
    (tmp_path / "b.obj").write_text("mtllib gone.mtl mesh.mtl\n" + body)  # two names, the first absent
    for name in ("a.obj", "b.obj"):
        assert np.array_equal(load_obj_textured(str(tmp_path / name))["texture"], img)


@pytest.mark.parametrize("mode", ["L", "RGBA", "LA", "P"])
def test_texture_images_become_rgb_uint8(tmp_path, mode):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    if mode in ("L", "LA"):
        rgb[..., 1] = rgb[..., 2] = rgb[..., 0]
    im = Image.fromarray(rgb, "RGB")
    if mode == "P":   # a palette image: lossless for at most 256 colours (35 here)
        im = im.quantize(colors=256)
        rgb = np.asarray(im.convert("RGB"))
    elif mode != "RGB":
        im = im.convert(mode)
        if "A" in mode:
            im.putalpha(Image.fromarray(rng.integers(0, 256, (5, 7), dtype=np.uint8), "L"))
    os.makedirs(tmp_path / "maps")
    im.save(str(tmp_path / "maps" / "skin.png"))
    m = load_obj_textured(_write(tmp_path, V + VT + "f 1/1 2/2 3/3\n"))
    assert m["texture"].shape == (5, 7, 3) and m["texture"].dtype == np.uint8
    assert np.array_equal(m["texture"], rgb)


def test_missing_pil_names_the_texture_argument(tmp_path, monkeypatch):
    import builtins
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(_lib.ScflowError, match="texture="):
        renderer.read_texture_image(str(tmp_path / "x.png"))


def test_load_meshes_obj_directory_brings_the_texture(tmp_path):
    pytest.importorskip("PIL")
    img = _rgb(6, 5)
    _png(str(tmp_path / "maps" / "skin.png"), img, "RGB")
    _write(tmp_path, V + VT + "f 1/1 2/2 3/3 4/4\n", name="obj_000003.obj")
    (tmp_path / "obj_000005.obj").write_text(V + "f 1 2 3\n")
    r = Renderer(mesh_dir=str(tmp_path), mesh_ext="obj", soft_blending=False, render_mask=False)
    assert sorted(r.meshes) == [2, 4] and sorted(r.textures) == [2]
    uv, fuv, tex = r.textures[2]
    assert tuple(uv.shape) == (6, 2) and fuv.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert np.array_equal(tex.numpy(), img)
    st = r.texture_store("cpu")
    assert st["offset"] == {2: 0} and st["hw"] == {2: (6, 5)}
    rgba = st["texels"].numpy().reshape(6, 5, 4)
    assert np.array_equal(rgba[..., :3], img) and (rgba[..., 3] == 255).all()


# ------------------------------------------------------------------------------------ add_mesh
def test_add_mesh_validation_and_registry():
    m = synthetic.textured_ellipsoid_mesh((50.0, 38.0, 30.0), 6, 8, (5, 4), seed=1)
    assert len(m["verts_uvs"]) > len(m["verts"]) and m["faces_uvs"].shape == m["faces"].shape
    assert m["texture"].dtype == np.uint8 and m["texture"].shape == (5, 4, 3)
    t = m["texture"]   # no symmetry under flips or transposition
    assert not np.array_equal(t, t[::-1]) and not np.array_equal(t, t[:, ::-1])
    sq = synthetic.textured_ellipsoid_mesh((1.0, 1.0, 1.0), 3, 3, (6, 6))["texture"]
    assert not np.array_equal(sq, sq.transpose(1, 0, 2))
    r = Renderer(soft_blending=False, render_mask=False)
    geo = (m["verts"], m["faces"], m["colors"])
    uv, fuv, tex = m["verts_uvs"], m["faces_uvs"], m["texture"]
    bad_idx = fuv.copy()
    bad_idx[3, 1] = len(uv)
    neg_idx = fuv.copy()
    neg_idx[0, 0] = -1
    for kw in (dict(verts_uvs=uv), dict(faces_uvs=fuv), dict(texture=tex),
               dict(verts_uvs=uv, faces_uvs=fuv), dict(verts_uvs=uv, texture=tex),
               dict(faces_uvs=fuv, texture=tex),
               dict(verts_uvs=uv, faces_uvs=fuv[:-1], texture=tex),
               dict(verts_uvs=uv, faces_uvs=fuv.astype(np.float32), texture=tex),
               dict(verts_uvs=uv, faces_uvs=bad_idx, texture=tex),
               dict(verts_uvs=uv, faces_uvs=neg_idx, texture=tex),
               dict(verts_uvs=uv[:, :1], faces_uvs=fuv, texture=tex),
               dict(verts_uvs=np.full_like(uv, np.nan), faces_uvs=fuv, texture=tex),
               dict(verts_uvs=uv, faces_uvs=fuv, texture=tex[..., 0]),
               dict(verts_uvs=uv, faces_uvs=fuv, texture=tex[:, :0]),
               dict(verts_uvs=uv, faces_uvs=fuv, texture=tex.astype(np.int32)),
               dict(verts_uvs=uv, faces_uvs=fuv, texture=tex.astype(np.float32))):  # floats > 1
        with pytest.raises(ValueError):
            r.add_mesh(0, *geo, **kw)
        assert not r.meshes and not r.textures and r._tex_store is None, kw
    r.add_mesh(0, *geo, verts_uvs=uv, faces_uvs=fuv, texture=tex)
    plain = Renderer(soft_blending=False, render_mask=False, meshes={0: geo})
    for k in range(4):   # verts, faces, colours, normals keep their places and values
        assert torch.equal(r.meshes[0][k], plain.meshes[0][k])
    assert len(r.meshes[0]) == 4 and r.meshes[0][1].dtype == torch.long
    assert np.array_equal(r.textures[0][2].numpy(), tex)
    # the meshes= constructor argument: a dict of add_mesh's keywords, or today's tuple
    r2 = Renderer(soft_blending=False, render_mask=False, meshes={0: m, 1: geo})
    assert sorted(r2.textures) == [0] and torch.equal(r2.textures[0][1], r.textures[0][1])
    # a float texture is quantised to round(x·255)
    r.add_mesh(1, *geo, verts_uvs=uv, faces_uvs=fuv, texture=np.array([[[0.0, 0.5, 1.0]]]))
    assert r.textures[1][2].tolist() == [[[0, 128, 255]]]
    # replacing a textured mesh by an untextured one drops its texture
    r.add_mesh(1, *geo)
    assert sorted(r.textures) == [0]


# ------------------------------------------------------------------ the restatement, pinned
def test_restatement_matches_closed_form_on_a_fronto_parallel_quad():
    """A quad parallel to the image plane with a texture that is affine in (row, col): the texel
    at pixel (r, c) is a closed-form affine function of (r, c).  OpenCV u of pixel column c is
    c0·(2c+1)/S (pytorch3d's sample positions), object x = (u − cx)·Z/fx, u_tex = (x + a)/2a, map
    x = u_tex·(W−1); v likewise with y down, so v = 1 — the file's FIRST row — at the quad's lower
    edge in the image, and map y = (1 − v_tex)·(H−1)."""
    import oracle.render_oracle as ro
    S, a, Z, fx, fy, cx, cy = 24, 50.0, 700.0, 150.0, 140.0, 11.0, 12.5
    H, W = 4, 5
    m = uvr.quad_mesh(a, uvr.ramp_texture(H, W))
    R, t = torch.eye(3, dtype=torch.float64), torch.tensor([3.0, -2.0, Z], dtype=torch.float64)
    K = torch.tensor([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=torch.float64)
    ndc = ro.project_ndc(torch.from_numpy(m["verts"]).double(), R, t, K, S)
    p2f, _, bary = ro.rasterize(ndc, torch.from_numpy(m["faces"]), S)
    hit = (p2f >= 0).numpy()
    assert hit.sum() > 150 and set(np.unique(p2f.numpy())) == {-1, 0, 1}
    got = uvr.texel_image(m, p2f, bary).numpy()
    rr, cc = np.mgrid[0:S, 0:S].astype(np.float64)
    c0 = (S - 1) / 2.0
    x_obj = (c0 * (2 * cc + 1) / S - cx) * Z / fx - 3.0
    y_obj = (c0 * (2 * rr + 1) / S - cy) * Z / fy + 2.0
    mx = (x_obj + a) / (2 * a) * (W - 1)
    my = (1.0 - (y_obj + a) / (2 * a)) * (H - 1)
    want = np.stack([10 + 3 * mx, 30 + 30 * my, 5 + 2 * mx + 9 * my], -1) / 255.0
    assert np.abs(got[hit] - want[hit]).max() <= 1e-9
    # orientation: the file's first row (G = 30/255) appears where v = 1, the image's lower edge
    rows = np.nonzero(hit.any(1))[0]
    col = int(np.nonzero(hit[rows[-1]])[0].mean())
    assert got[rows[-1], col, 1] < 45 / 255.0 and got[rows[0], col, 1] > 105 / 255.0
    # and the border clamp: uv·1.6 − 0.3 saturates at the first / last texel
    wide = dict(m, verts_uvs=m["verts_uvs"] * np.float32(1.6) - np.float32(0.3))
    gw = uvr.texel_image(wide, p2f, bary).numpy()[hit]
    assert abs(gw[:, 0].min() - 10 / 255.0) < 1e-15 and abs(gw[:, 0].max() - (10 + 3 * (W - 1)) / 255.0) < 1e-15


def test_direct_formula_equals_grid_sample():
    """The formula of include/scflow_hip.h (x = clamp(u·(W−1)), y = clamp((1−v)·(H−1)), upper taps
    clamped) against pytorch3d's formulation (flip + grid_sample), fp64, uv in [−0.3, 1.3] and the
    corners."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for h, w in uvr.MAPS:
        tex = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        uv = np.concatenate([rng.uniform(-0.3, 1.3, (500, 2)), [[0, 0], [1, 0], [0, 1], [1, 1]]])
        x = np.clip(uv[:, 0] * (w - 1), 0, w - 1)
        y = np.clip((1 - uv[:, 1]) * (h - 1), 0, h - 1)
        x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        fx, fy = (x - x0)[:, None], (y - y0)[:, None]
        T = tex.astype(np.float64) / 255.0
        want = (T[y0, x0] * (1 - fx) + T[y0, x1] * fx) * (1 - fy) + (T[y1, x0] * (1 - fx) + T[y1, x1] * fx) * fy
        worst = max(worst, np.abs(uvr.sample_textures(tex, uv).numpy() - want).max())
    assert worst <= 1e-13, worst


# ------------------------------------------------------------------------------------ C ABI
def test_render_tex_struct_layout_matches_header(tmp_path):
    _layout(tmp_path, "RenderTex", "scflow_render_tex")


def test_render_textured_is_a_new_export_only():
    lib = _lib.load()
    assert lib.scflow_abi_version() == 4 == _lib.ABI_VERSION
    src = open(os.path.join(ROOT, "include", "scflow_hip.h")).read()
    assert "#define SCFLOW_ABI_VERSION 4\n" in src
    assert lib.scflow_render_textured(None, None, None) == -1   # SCFLOW_EINVAL, nothing launched
    assert lib.scflow_render_textured(None, ctypes.byref(_lib.RenderTex()), None) == -1
