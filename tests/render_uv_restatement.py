"""Test-side helper (not a test): an fp64 restatement of how pytorch3d shades a UV-textured mesh
(``TexturesUV.sample_textures`` behind ``HardPhongShader``, pytorch3d 0.7, with its defaults
``align_corners=True``, ``padding_mode='border'``, ``sampling_mode='bilinear'``), for the tests of
``scflow_render_textured`` (tests/test_render_uv_host.py, tests/test_gpu_render_uv.py).

It shades given fragments (pix_to_face, barycentrics); it does not rasterise —
``oracle/render_oracle.py::rasterize`` and tests/render_cases.py do.

* Texels are taken the way pytorch3d takes them, not the way the kernel does: the map's rows are
  flipped, uv goes to uv·2 − 1, and ``torch.nn.functional.grid_sample`` samples.  The kernel uses
  the direct formula on the unflipped map (include/scflow_hip.h).
* Positions and normals are interpolated, and the light applied, by ``render_oracle.phong``
  itself: called with vertex colours 1 and 0 it returns (ambient + diffuse·dif) + specular·spec
  and specular·spec, from which rgb = (ambient + diffuse·dif)·texel + specular·spec follows.

Parity with pytorch3d itself is unpinned (it is not installed); the restatement is pinned to a
closed form on a fronto-parallel quad (tests/test_render_uv_host.py).

Also here: the scenes the CPU and GPU tests share (``quad_mesh``, ``sampling_scene``).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle.render_oracle as ro
from scflow_amd import synthetic

MAPS = ((1, 1), (2, 3), (5, 4), (16, 16), (7, 64))   # (H, W): the non-square ones catch swapped axes


def sample_textures(texture, uv):
    """pytorch3d's sampling: ``texture`` [H, W, 3] uint8 (row 0 = the file's first row), ``uv``
    [..., 2] → texels [..., 3] float64."""
    tmap = torch.as_tensor(np.asarray(texture)).double().div(255.0).permute(2, 0, 1)[None]  # [1,3,H,W]
    tmap = torch.flip(tmap, [2])                       # "flip y axis of the texture map"
    uv = torch.as_tensor(uv, dtype=torch.float64)
    grid = (uv * 2.0 - 1.0).reshape(1, -1, 1, 2)
    out = F.grid_sample(tmap, grid, mode="bilinear", align_corners=True, padding_mode="border")
    return out[0, :, :, 0].T.reshape(*uv.shape[:-1], 3)


def pixel_uvs(mesh, p2f, bary):
    """uv = Σ b_k · verts_uvs[faces_uvs[f][k]] at every pixel ([S,S,2] float64; 0 where empty)."""
    p2f = torch.as_tensor(np.asarray(p2f)).long()
    bary = torch.as_tensor(np.asarray(bary)).double()
    uv = torch.as_tensor(np.asarray(mesh["verts_uvs"])).double()
    fuv = torch.as_tensor(np.asarray(mesh["faces_uvs"])).long()
    corner = uv[fuv[p2f.clamp(min=0)]]                 # [S, S, 3 corners, 2]
    out = (bary[..., :, None] * corner).sum(-2)
    return torch.where((p2f >= 0)[..., None], out, torch.zeros_like(out))


def texel_image(mesh, p2f, bary):
    """The texel every pixel's fragment samples ([S,S,3] float64; arbitrary where empty)."""
    return sample_textures(mesh["texture"], pixel_uvs(mesh, p2f, bary))


LIGHT_COLOURS = {True: dict(ambient=0.5, diffuse=0.3, specular=0.2),    # default_lights
                 False: dict(ambient=0.8, diffuse=0.5, specular=1.0)}


def shade_image(mesh, p2f, bary, R, t, light, background=(0.5, 0.5, 0.5), shininess=64.0,
                ambient=0.5, diffuse=0.3, specular=0.2):
    """HardPhongShader on the fragments of one image → [S,S,4] float64.  ``mesh``: dict(verts,
    faces, colors, and verts_uvs / faces_uvs / texture or None for those), ``p2f`` [S,S] the
    mesh's own face indices (−1 empty), ``light`` [3] the light location, R / t the OpenCV pose."""
    T = lambda a: torch.as_tensor(np.asarray(a)).double()  # noqa: E731
    verts, faces = T(mesh["verts"]), torch.as_tensor(np.asarray(mesh["faces"])).long()
    p2f, bary = torch.as_tensor(np.asarray(p2f)).long(), T(bary)
    R, t = T(R), T(t)
    args = (p2f, bary, T(light), -R.T @ t, background, shininess, ambient, diffuse, specular)
    normals = ro.verts_normals(verts, faces)
    if mesh.get("texture") is None:
        return ro.phong(verts, faces, normals, T(mesh["colors"]), *args)
    lit1 = ro.phong(verts, faces, normals, torch.ones_like(verts), *args)   # (amb + dif) + spec
    lit0 = ro.phong(verts, faces, normals, torch.zeros_like(verts), *args)  # spec
    rgb = (lit1[..., :3] - lit0[..., :3]) * texel_image(mesh, p2f, bary) + lit0[..., :3]
    rgb = torch.where((p2f >= 0)[..., None], rgb, lit1[..., :3])            # background
    return torch.cat([rgb, lit1[..., 3:]], -1)


# ------------------------------------------------------------------------------------ scenes
def ramp_texture(h, w):
    """uint8 [h, w, 3], affine in (row, col) exactly: R = 10 + 3·col, G = 30 + 30·row,
    B = 5 + 2·col + 9·row (h ≤ 7, w ≤ 64)."""
    row, col = np.mgrid[0:h, 0:w]
    tex = np.stack([10 + 3 * col, 30 + 30 * row, 5 + 2 * col + 9 * row], -1)
    assert tex.max() <= 255
    return tex.astype(np.uint8)


def quad_mesh(a=50.0, texture=None):
    """A square of side 2a in the plane z = 0, two triangles, UV corners (0,0), (1,0), (1,1),
    (0,1) at (−a,−a), (a,−a), (a,a), (−a,a); the winding faces a camera that looks along +z."""
    verts = np.array([[-a, -a, 0], [a, -a, 0], [a, a, 0], [-a, a, 0]], np.float32)
    faces = np.array([[0, 2, 1], [0, 3, 2]], np.int64)
    return dict(verts=verts, faces=faces, colors=np.full((4, 3), 0.5, np.float32),
                verts_uvs=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32),
                faces_uvs=faces.copy(), texture=ramp_texture(4, 5) if texture is None else texture)


def noise_texture(h, w, seed=0):
    """The asymmetric texture of ``synthetic.textured_ellipsoid_mesh`` at (h, w)."""
    return synthetic.textured_ellipsoid_mesh((1.0, 1.0, 1.0), 3, 3, (h, w), seed)["texture"]


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = (f(v) for v in (ax, ay, az) for f in (math.cos, math.sin))
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


# the ellipsoid's seam (longitude 0, the +x axis) turned towards the camera and tilted: faces on
# both sides of the seam, and a pole's fan, are visible
SEAM_R = _rot(0.5, math.radians(100.0), 0.2)
QUAD_R = _rot(0.35, -0.3, 0.15)   # a slanted quad: the uv interpolation is perspective-corrected


def sampling_scene(S):
    """The batch of the sampling tests at image size S: for every map size of ``MAPS``, the quad and
    the 6×8 textured ellipsoid, each with its own uv and with uv·1.6 − 0.3 (reaching [−0.3, 1.3]:
    the border clamp).  dict(meshes [list of dicts], R, t, K float32, tags)."""
    meshes, Rs, ts, tags = [], [], [], []
    for i, (h, w) in enumerate(MAPS):
        for wide in (False, True):
            q = quad_mesh(50.0, noise_texture(h, w, seed=i))
            e = synthetic.textured_ellipsoid_mesh((50.0, 38.0, 30.0), 6, 8, (h, w), seed=10 + i)
            for name, m, R in (("quad", q, QUAD_R), ("ell", e, SEAM_R)):
                if wide:
                    m = dict(m, verts_uvs=(m["verts_uvs"] * np.float32(1.6) - np.float32(0.3)))
                meshes.append(m)
                Rs.append(R)
                ts.append([2.0, -3.0, 700.0])
                tags.append(f"{name}-{h}x{w}{'-wide' if wide else ''}")
    f = 0.2 * 700.0 * S / 24.0
    K = np.array([[f, 0, (S - 1) / 2 + 0.3], [0, 1.1 * f, (S - 1) / 2 - 0.2], [0, 0, 1]])
    n = len(meshes)
    return dict(meshes=meshes, R=np.stack(Rs).astype(np.float32), t=np.array(ts, np.float32),
                K=np.repeat(K[None], n, 0).astype(np.float32), tags=tags)


def seam_faces(n_lat, n_lon):
    """Indices of the faces of ``textured_ellipsoid_mesh(·, n_lat, n_lon)`` that touch the seam
    column (a vertex at longitude 0), poles excluded from the vertex set."""
    _, faces, _ = synthetic.ellipsoid_mesh((1.0, 1.0, 1.0), n_lat, n_lon)
    seam_verts = 1 + (np.arange(1, n_lat) - 1) * n_lon
    return np.nonzero(np.isin(faces, seam_verts).any(1))[0]


def per_vertex_uvs(mesh, n_lat, n_lon):
    """The per-vertex emulation of the seam: every corner at a seam vertex gets that vertex's one
    texture coordinate (u = 0), also on the side where the unwrapping says u = 1."""
    fuv = np.array(mesh["faces_uvs"])
    for i in range(1, n_lat):
        fuv[fuv == (i - 1) * (n_lon + 1) + n_lon] = (i - 1) * (n_lon + 1)
    return dict(mesh, faces_uvs=fuv)
