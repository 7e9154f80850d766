"""GPU: the HIP renderer (scflow_render) against the oracle restatement of pytorch3d's
rasteriser + hard Phong shader (oracle/render_oracle.py; parity with pytorch3d itself is
UNPINNED — it is absent — the oracle is pinned to closed-form ellipsoid depth in
tests/test_render_host.py), and directly against the closed-form depth at 256².

Tolerances: pix_to_face equal on ≥ 99.7 % of pixels (the rest are fp32 vs fp64 decisions on
pixel centres within rounding of a shared edge), zbuf relative 1e-5 and RGB 2e-3 absolute on the
pixels where both pick the same face (barycentrics 1e-3: fp32 edge functions of small
triangles in NDC cancel); coverage equal to the oracle's on ≥ 99.7 %.

On top of that blanket allowance every differing pixel has to be explained by the per-pixel rule
of tests/render_cases.py (the kernel's face a legitimate contender in fp64, the oracle's face on
an edge or in a depth near-tie; explained pixels capped per image at max(2, 0.1 % of S²)), here
and on that module's edge scenes: silhouettes across image borders, partial 16×16 tiles (S = 24,
40, 56, 72), a fully covered and an empty image, 12-face to 1840-face meshes in one batch, five
images in one wave of the projection kernel, a torus, interpenetrating surfaces with exact depth
ties.  Measured on the MI355X: 0 differing pixels on every image (109 edge-scene renders, 20
``make_scene`` renders), so no pixel needed the rule; largest differences on the edge scenes
zbuf 6.2e-7 relative, barycentrics 3.6e-5, RGBA 6.4e-6, and on ``make_scene`` (S = 128) zbuf
2.8e-6, barycentrics 6.7e-4, RGBA 1.7e-5.  Batch vs single-image renders, repeated renders and
renders without the image are bit-identical."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ro = pytest.importorskip("oracle.render_oracle")
from tests import render_cases as rc  # noqa: E402


def _meshes():
    from scflow_amd import synthetic
    out = {}
    for lab in (3, 7):
        semi = np.array(synthetic.ELLIPSOID_AXES) * synthetic.YCBV_DIAMETERS[lab]
        out[lab] = synthetic.ellipsoid_mesh(semi, 16 + 4 * (lab % 4), 32)
    return out


def _to_numpy(out):
    """A Renderer result → the batch arrays of tests/render_cases.py (packed pix_to_face)."""
    fr = out["fragments"]
    return dict(p2f=fr.pix_to_face[..., 0].cpu().numpy(), zbuf=fr.zbuf[..., 0].cpu().numpy(),
                bary=fr.bary_coords[..., 0, :].cpu().numpy(),
                images=out["images"].cpu().numpy() if "images" in out else None)


def _render_batch(b, light=(True, True), idx=None, render_image=True):
    """The images ``idx`` (all by default) of a tests/render_cases.py batch through the HIP
    Renderer, in one call: (Renderer result, face offsets of that call's packed faces)."""
    from scflow_amd.renderer import Renderer
    idx = list(range(len(b["names"]))) if idx is None else idx
    r = Renderer(image_size=(b["S"], b["S"]), soft_blending=False, render_mask=False,
                 render_image=render_image, seperate_lights=light[0], default_lights=light[1],
                 meshes={i: tuple(np.array(x) for x in b["meshes"][i]) for i in idx}).to("cuda")
    out = r(*(torch.from_numpy(b[k][idx]).cuda() for k in ("R", "t", "K", "labels")))
    torch.cuda.synchronize()
    off = np.concatenate([[0], np.cumsum([len(b["meshes"][i][1]) for i in idx])])
    return out, off


@pytest.mark.parametrize("S,seps,deflt", [(64, True, True), (128, True, True), (64, False, True),
                                          (64, True, False), (64, False, False)])
def test_render_matches_oracle(S, seps, deflt):
    from scflow_amd import synthetic
    from scflow_amd.renderer import Renderer
    meshes = _meshes()
    sc = synthetic.make_scene(4, S, seed=11)
    labels = np.array([3, 7, 3, 7])
    r = Renderer(image_size=(S, S), soft_blending=False, render_mask=False, seperate_lights=seps,
                 default_lights=deflt, meshes=meshes).to("cuda")
    R, t, K = (torch.from_numpy(sc[k]) for k in ("ref_rotation", "ref_translation", "internel_k"))
    out = r(R.cuda(), t.cuda(), K.cuda(), torch.from_numpy(labels).cuda())
    torch.cuda.synchronize()
    om = {lab: tuple(torch.from_numpy(x).double() if x.dtype != np.int64 else torch.from_numpy(x)
                     for x in m) for lab, m in meshes.items()}
    imgs, zbuf, p2f, bary = ro.render(om, R.double(), t.double(), K.double(), labels.tolist(), S,
                                      light=(seps, deflt))
    g_p2f = out["fragments"].pix_to_face[..., 0].cpu()
    same = g_p2f == p2f
    assert same.float().mean() >= 0.997
    assert ((g_p2f >= 0) == (p2f >= 0)).float().mean() >= 0.997
    hit = same & (p2f >= 0)
    assert hit.sum() > 100
    gz = out["fragments"].zbuf[..., 0].cpu().double()
    np.testing.assert_allclose(gz[hit].numpy(), zbuf[hit].numpy(), rtol=1e-5)
    assert (gz[p2f < 0][g_p2f[p2f < 0] < 0] == -1).all()
    gb = out["fragments"].bary_coords[..., 0, :].cpu().double()
    np.testing.assert_allclose(gb[hit].numpy(), bary[hit].numpy(), atol=1e-3)
    gi = out["images"].cpu().double()
    np.testing.assert_allclose(gi[hit].numpy(), imgs[hit].numpy(), atol=2e-3)
    bg = (p2f < 0) & (g_p2f < 0)
    np.testing.assert_allclose(gi[bg].numpy(), imgs[bg].numpy(), atol=0)
    # the per-pixel rule on every differing pixel (tests/render_cases.py)
    off = np.concatenate([[0], np.cumsum([len(meshes[int(l)][1]) for l in labels])])
    got = rc.split_batch(_to_numpy(out), off)
    orc = rc.split_batch(dict(p2f=p2f.numpy(), zbuf=zbuf.numpy(), bary=bary.numpy(),
                              images=imgs.numpy()), off)
    ndcs = [rc.project64(meshes[int(l)][0], sc["ref_rotation"][i], sc["ref_translation"][i],
                         sc["internel_k"][i], S) for i, l in enumerate(labels)]
    rc.compare_batch(f"make_scene S={S} light {(seps, deflt)}", got, orc, ndcs, meshes, labels, S)


def test_render_depth_matches_closed_form_256():
    """Finely tessellated stand-in object at the bench resolution: the HIP z-buffer against the
    ray/ellipsoid depth at pytorch3d's sample positions (faceting error only)."""
    from scflow_amd import synthetic
    from scflow_amd.renderer import Renderer
    from tests.test_render_host import analytic_depth
    S = 256
    sc = synthetic.make_scene(2, S, seed=5)
    meshes, refs = {}, []
    for i, lab in enumerate(sc["labels"].tolist()):
        semi = np.array(synthetic.ELLIPSOID_AXES) * synthetic.YCBV_DIAMETERS[lab]
        meshes[lab] = synthetic.ellipsoid_mesh(semi, 128, 256)
        refs.append(analytic_depth(sc["ref_rotation"][i].astype(np.float64),
                                   sc["ref_translation"][i].astype(np.float64),
                                   sc["internel_k"][i].astype(np.float64), S, semi))
    r = Renderer(image_size=(S, S), soft_blending=False, render_mask=False, seperate_lights=True,
                 meshes=meshes).to("cuda")
    out = r(*(torch.from_numpy(sc[k]).cuda() for k in ("ref_rotation", "ref_translation",
                                                       "internel_k", "labels")))
    z = out["fragments"].zbuf[..., 0].cpu().numpy()
    for i, (zr, hit) in enumerate(refs):
        cov = z[i] > 0
        assert (cov != hit).mean() < 0.01
        both = cov & hit
        rel = np.abs(z[i][both] - zr[both]) / zr[both]
        assert np.median(rel) < 1e-4 and rel.max() < 2e-3


def test_refiner_render_and_refine_cycles():
    """SCFlowRefiner with a renderer config: ``render`` = the Renderer's image / zbuf / mask
    (format_data_test's render step), and ``refine`` (render → get_pose per cycle) with one
    cycle equals get_pose on the rendered inputs; two cycles re-render at the refined pose."""
    from scflow_amd import MODELS, synthetic
    from tests.test_gpu_decoder import decoder_cfg
    from tests.test_gpu_encoder import encoder_state_dict  # noqa: F401  (same weights as the e2e tests)
    from tests.helpers import refiner_state_dict
    S, B = 256, 2
    sc = synthetic.make_scene(B, S, seed=21)
    meshes = {}
    for lab in set(sc["labels"].tolist()):
        semi = np.array(synthetic.ELLIPSOID_AXES) * synthetic.YCBV_DIAMETERS[lab]
        meshes[lab] = synthetic.ellipsoid_mesh(semi, 24, 48)
    enc = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic", norm_cfg=dict(type="IN"))
    ctx = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic", norm_cfg=dict(type="BN"))
    r = MODELS.build(dict(type="SCFlowRefiner", cxt_channels=128, h_channels=128, seperate_encoder=False,
                          encoder=enc, cxt_encoder=ctx, decoder=dict(type="SCFlowDecoder", **decoder_cfg(2)),
                          renderer=dict(mesh_dir=None, image_size=(S, S), soft_blending=False,
                                        render_mask=False, seperate_lights=True, meshes=meshes),
                          test_cfg=dict(iters=2, cycles=2)))
    r.load_state_dict({("decoder." + k if not k.startswith(("real_encoder.", "render_encoder.", "context."))
                        else k): v for k, v in refiner_state_dict().items()}, strict=False)
    r = r.eval().cuda()
    R, t, K, lab = (torch.from_numpy(sc[k]).cuda() for k in ("ref_rotation", "ref_translation",
                                                             "internel_k", "labels"))
    tgt = synthetic.make_train_targets(sc, S, seed=21)
    real, _, _ = r.render(torch.from_numpy(tgt["gt_rotation"]).cuda(),
                          torch.from_numpy(tgt["gt_translation"]).cuda(), K, lab)
    img, depth, mask = r.render(R, t, K, lab)
    direct = r.renderer(R, t, K, lab)
    torch.testing.assert_close(img, direct["images"][..., :3].permute(0, 3, 1, 2))
    torch.testing.assert_close(depth, direct["fragments"].zbuf[..., 0])
    assert ((depth > 0) == (mask > 0)).all() and mask.sum() > 1000
    R1, t1, out1 = r.refine(real, R, t, K, lab, cycles=1)
    ref_out = r.get_pose(img, real, R, t, depth, K, lab)
    torch.testing.assert_close(R1, ref_out[2][-1])
    torch.testing.assert_close(t1, ref_out[3][-1])
    R2, t2, _ = r.refine(real, R, t, K, lab)  # test_cfg cycles = 2
    torch.cuda.synchronize()
    assert torch.isfinite(R2).all() and torch.isfinite(t2).all()
    assert not torch.equal(R2, R1)


@pytest.mark.parametrize("deflt,seps", [(True, True), (True, False), (False, True), (False, False)])
def test_kernel_light_location_matches_reference_fixture(deflt, seps):
    """The light each image is shaded with (scflow_render's light_out) against the PointLights
    location the reference's own Renderer.forward builds (golden_render_wiring.npz, rendering.py:
    209-230; tests/test_render_wiring.py pins the rest of the wiring on the CPU)."""
    from scflow_amd import synthetic
    from scflow_amd.renderer import Renderer
    from tests.helpers import golden
    gd = golden("render_wiring")
    labels = gd["in_labels"]
    meshes = {int(l): synthetic.ellipsoid_mesh(np.array(synthetic.ELLIPSOID_AXES) *
                                               synthetic.YCBV_DIAMETERS[int(l)], 12, 24)
              for l in set(labels.tolist())}
    S = int(gd["in_S"])
    r = Renderer(image_size=(S, S), soft_blending=False, render_mask=False, seperate_lights=seps,
                 default_lights=deflt, meshes=meshes).to("cuda")
    out = r(*(torch.from_numpy(gd[k]).cuda() for k in ("in_R", "in_t", "in_K", "in_labels")))
    got = out["light_location"].cpu().numpy()
    rec = gd[f"d{int(deflt)}s{int(seps)}_light_location"]
    if rec.size == 0:  # PointLights() default location (pytorch3d's (0, 1, 0))
        rec = np.tile([0.0, 1.0, 0.0], (len(labels), 1))
    np.testing.assert_allclose(got, rec, rtol=1e-5, atol=1e-3)


# ------------------------------------------------------------------ edge scenes (render_cases.py)
_EDGE = [(name, seed, light) for name in rc.BATCHES for seed in rc.SEEDS
         for light in (rc.LIGHTS if name in ("s40", "s24") else rc.LIGHTS[:1])]


@pytest.mark.parametrize("name,seed,light", _EDGE,
                         ids=[f"{n}-seed{s}-sep{int(l[0])}def{int(l[1])}" for n, s, l in _EDGE])
def test_render_edge_scenes(name, seed, light):
    """Borders, partial tiles, tiny / non-convex meshes, ragged batches: the Renderer against the
    fp64 oracle under the per-pixel rule, and the light each image is shaded with."""
    b = rc.batch(name, seed)
    out, off = _render_batch(b, light)
    got = rc.split_batch(_to_numpy(out), off)
    rc.compare_batch(f"hip {name} seed {seed} light {light}", got, rc.oracle(name, seed, light),
                     rc.ndc64(name, seed), b["meshes"], b["labels"], b["S"], names=b["names"])
    np.testing.assert_allclose(out["light_location"].cpu().numpy(), rc.lights64(name, seed, light),
                               rtol=1e-5, atol=1e-3)
    if name == "double48":   # exact ties go to the lower face index
        _, (f1, f2) = rc.double_ellipsoid()
        assert (got[0]["p2f"] < f1 + f2).all()
    if name == "s40":        # the empty image, whatever the oracle says
        e = got[b["names"].index("offscreen")]
        assert (e["p2f"] == -1).all() and (e["zbuf"] == -1).all() and (e["bary"] == -1).all()
        assert (e["images"][..., :3] == 0.5).all() and (e["images"][..., 3] == 0).all()


@pytest.mark.parametrize("name", ["s40", "s24"])
def test_render_batch_equals_single_images(name):
    """Each image rendered alone is bit-identical to its slice of the batch render (face ranges,
    per-image minimum depth: nothing leaks between the images of a batch)."""
    b = rc.batch(name, 0)
    out, off = _render_batch(b, (True, True))
    whole = rc.split_batch(_to_numpy(out), off)
    lights = out["light_location"].cpu().numpy()
    for i, nm in enumerate(b["names"]):
        one, off1 = _render_batch(b, (True, True), idx=[i])
        single = rc.split_batch(_to_numpy(one), off1)[0]
        for k in ("p2f", "zbuf", "bary", "images"):
            assert np.array_equal(single[k], whole[i][k]), (nm, k)
        assert np.array_equal(one["light_location"].cpu().numpy()[0], lights[i]), nm


@pytest.mark.parametrize("name", ["s24", "chunks72"])
def test_render_repeatable(name):
    """Two calls on the same inputs are bit-identical: the order in which a tile's faces land in
    LDS does not matter."""
    b = rc.batch(name, 1)
    a1, a2 = _to_numpy(_render_batch(b)[0]), _to_numpy(_render_batch(b)[0])
    for k in ("p2f", "zbuf", "bary", "images"):
        assert np.array_equal(a1[k], a2[k]), k


def test_render_without_image():
    b = rc.batch("s40", 1)
    full, geo = _render_batch(b)[0], _render_batch(b, render_image=False)[0]
    assert "images" not in geo and "images" in full
    a1, a2 = _to_numpy(full), _to_numpy(geo)
    for k in ("p2f", "zbuf", "bary"):
        assert np.array_equal(a1[k], a2[k]), k
    assert torch.equal(full["light_location"], geo["light_location"])


def test_render_rejects_bad_arguments():
    """scflow_render through the C ABI: a workspace 16 bytes short, n_img = 0 and light_mode = 3
    return non-zero and write nothing (every pointer stays valid and every buffer full-sized)."""
    import ctypes
    from scflow_amd import _lib
    from scflow_amd.renderer import verts_normals
    lib = _lib.load()
    b = rc.batch("s24", 0)
    n, S = len(b["names"]), b["S"]
    ms = [b["meshes"][i] for i in range(n)]
    nv, nf = [len(m[0]) for m in ms], [len(m[1]) for m in ms]
    voff = np.concatenate([[0], np.cumsum(nv)[:-1]])
    dev = "cuda"
    verts = torch.from_numpy(np.concatenate([m[0] for m in ms])).to(dev)
    colors = torch.from_numpy(np.concatenate([m[2] for m in ms])).to(dev)
    normals = torch.cat([verts_normals(torch.from_numpy(np.array(m[0])).double(),
                                       torch.from_numpy(np.array(m[1]))).float() for m in ms]).to(dev)
    faces = torch.from_numpy(np.concatenate([m[1] + o for m, o in zip(ms, voff)])).to(torch.int32).to(dev)
    vert_img = torch.from_numpy(np.repeat(np.arange(n), nv)).to(torch.int32).to(dev)
    face_img = torch.from_numpy(np.repeat(np.arange(n), nf)).to(torch.int32).to(dev)
    R, t, K = (torch.from_numpy(np.array(b[k])).to(dev).contiguous() for k in ("R", "t", "K"))
    need = int(lib.scflow_render_workspace(n, S, verts.shape[0]))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    params = torch.tensor([0.5] * 3 + [0.3] * 3 + [0.2] * 3 + [0.5] * 3 + [0.0, 1.0, 0.0], device=dev)
    sentinel = 777.0
    images = torch.full((n, S, S, 4), sentinel, device=dev)
    zbuf = torch.full((n, S, S), sentinel, device=dev)
    p2f = torch.full((n, S, S), 777, device=dev, dtype=torch.int32)
    bary = torch.full((n, S, S, 3), sentinel, device=dev)
    light = torch.full((n, 3), sentinel, device=dev)

    def args(**over):
        a = _lib.RenderArgs()
        a.verts, a.normals, a.colors, a.faces = (verts.data_ptr(), normals.data_ptr(),
                                                 colors.data_ptr(), faces.data_ptr())
        a.vert_img, a.face_img = vert_img.data_ptr(), face_img.data_ptr()
        a.R, a.t, a.K = R.data_ptr(), t.data_ptr(), K.data_ptr()
        a.n_img, a.size, a.total_verts, a.total_faces = n, S, verts.shape[0], faces.shape[0]
        a.light_mode = _lib.SCFLOW_LIGHT_PER_IMAGE
        base = params.data_ptr()
        a.ambient, a.diffuse, a.specular, a.background = base, base + 12, base + 24, base + 36
        a.light_location = base + 48
        a.shininess = 64.0
        a.images, a.zbuf, a.pix_to_face, a.bary = (images.data_ptr(), zbuf.data_ptr(),
                                                   p2f.data_ptr(), bary.data_ptr())
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        a.light_out = light.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a
    stream = torch.cuda.current_stream().cuda_stream
    for over in (dict(workspace_bytes=need - 16), dict(n_img=0), dict(light_mode=3)):
        a = args(**over)
        assert lib.scflow_render(ctypes.byref(a), stream) != 0, over
        torch.cuda.synchronize()
        assert (zbuf == sentinel).all() and (p2f == 777).all() and (bary == sentinel).all(), over
        assert (images == sentinel).all() and (light == sentinel).all() and (ws == 0).all(), over
    a = args()   # the same arguments, unbroken, render
    assert lib.scflow_render(ctypes.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert (zbuf != sentinel).all() and (images != sentinel).all() and (light != sentinel).all()
    got = rc.split_batch(dict(p2f=p2f.cpu().numpy(), zbuf=zbuf.cpu().numpy(), bary=bary.cpu().numpy(),
                              images=images.cpu().numpy()), b["face_offset"])
    rc.compare_batch("hip s24 through the C ABI", got, rc.oracle("s24", 0), rc.ndc64("s24", 0),
                     b["meshes"], b["labels"], S, names=b["names"])
