"""GPU: ``patches.frames_to_train_patches`` and ``SCFlowRefiner.train_batch_from_frames`` on the
synthetic 300×400 frames of tests/test_gpu_patch_refiner.py (256² renders of the synthetic scene
pasted at known offsets): frames, GT poses and masks in, a ``TrainStep`` batch and a loss out."""
from functools import lru_cache

import numpy as np
import pytest
import torch

pytest.importorskip("oracle.scflow_oracle")
pytestmark = pytest.mark.gpu

S, FH, FW = 256, 300, 400
OFFSETS = [(100, 30), (20, 44)]
SEED, STEP = 99, 4
QUIET = dict(angle_std=0.0, x_std=0.0, y_std=0.0, z_std=0.0, p_hsv=0.0, p_noise=0.0, p_blur=0.0)


@lru_cache(maxsize=None)
def setup():
    from scflow_amd import synthetic
    from tests.test_train_host import build_train_refiner
    sc = synthetic.make_scene(2, S, seed=21)
    meshes = {}
    for lab in set(sc["labels"].tolist()):
        semi = np.array(synthetic.ELLIPSOID_AXES) * synthetic.YCBV_DIAMETERS[lab]
        meshes[lab] = synthetic.ellipsoid_mesh(semi, 24, 48)
    r = build_train_refiner(2, renderer=dict(mesh_dir=None, image_size=(S, S), soft_blending=False,
                                             render_mask=False, seperate_lights=True,
                                             meshes=meshes)).cuda()
    K, lab = (torch.from_numpy(sc[k]).cuda() for k in ("internel_k", "labels"))
    tgt = synthetic.make_train_targets(sc, S, seed=21)
    Rg, tg = (torch.from_numpy(tgt[k]).cuda() for k in ("gt_rotation", "gt_translation"))
    real, _, _ = r.render(Rg, tg, K, lab)
    bgr = (real.flip(1) * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    frames = torch.full((2, FH, FW, 3), 128, dtype=torch.uint8, device="cuda")
    ori_k = K.clone()
    for i, (ox, oy) in enumerate(OFFSETS):
        frames[i, oy:oy + S, ox:ox + S] = bgr[i]
        ori_k[i, 0, 2] += ox
        ori_k[i, 1, 2] += oy
    masks = (frames != 128).any(-1).to(torch.uint8).contiguous()
    diam = torch.tensor(synthetic.YCBV_DIAMETERS, dtype=torch.float32, device="cuda")
    return dict(refiner=r, Rg=Rg, tg=tg, labels=lab, frames=frames.contiguous(), masks=masks,
                ori_k=ori_k, fidx=torch.arange(2, device="cuda"), diam=diam)


def batch_of(s, **kw):
    return s["refiner"].train_batch_from_frames(s["frames"], s["masks"], s["fidx"], s["Rg"], s["tg"],
                                                s["ori_k"], s["labels"], s["diam"], SEED, STEP, **kw)


def test_without_jitter_and_stages_it_is_frames_to_patches_at_the_drawn_ratio():
    from scflow_amd import patches
    s = setup()
    b = batch_of(s, aug=QUIET)
    assert b["valid"].tolist() == [True, True] and (b["aug"][:, 5] == 0).all()
    assert torch.equal(b["ref_rotation"], s["Rg"]) and torch.equal(b["ref_translation"], s["tg"])
    assert not b["init_rot_error"].any() and not b["init_trans_error"].any()
    assert ((b["ratio"] >= 1.0) & (b["ratio"] < 1.25)).all() and b["ratio"][0] != b["ratio"][1]
    points, counts = patches.point_table(s["refiner"].renderer)
    d = patches.frames_to_patches(s["frames"], s["fidx"], s["Rg"], s["tg"], s["ori_k"], s["labels"],
                                  points, counts, size=S, size_ratio=b["ratio"])
    for key in ("real_images", "internel_k", "transform_matrix", "geom"):
        assert torch.equal(b[key], d[key]), key
    assert b["real_images"].std() > 0.05
    m = patches.extract_maps(s["masks"], s["fidx"], d["geom"], d["valid"], S, mode="nearest")[:, 0]
    assert torch.equal(b["gt_masks"], (m > 0).float()) and 0.2 < float(b["gt_masks"].mean()) < 0.9


def test_train_batch_is_what_train_step_reads():
    from scflow_amd import patches, synthetic
    from scflow_amd.train.step import TrainStep
    s = setup()
    r = s["refiner"]
    b = batch_of(s)
    f32 = torch.float32
    want = dict(real_images=((2, 3, S, S), f32), render_images=((2, 3, S, S), f32),
                depth=((2, S, S), f32), internel_k=((2, 3, 3), f32), ref_rotation=((2, 3, 3), f32),
                ref_translation=((2, 3), f32), gt_rotation=((2, 3, 3), f32),
                gt_translation=((2, 3), f32), label=((2,), torch.int64), gt_masks=((2, S, S), f32),
                valid=((2,), torch.bool), init_add_error=((2,), f32), init_rot_error=((2,), f32),
                init_trans_error=((2,), f32), aug=((2, 8), f32), geom=((2, 8), torch.int32),
                transform_matrix=((2, 3, 3), f32))
    for key, (shape, dtype) in want.items():
        assert tuple(b[key].shape) == shape and b[key].dtype == dtype, key
    assert b["valid"].all() and (b["init_rot_error"] > 0).all() and (b["init_rot_error"] <= 45).all()
    assert (b["init_trans_error"] <= 200).all() and (b["init_add_error"] <= 1).all()
    assert not torch.equal(b["ref_rotation"], s["Rg"]) and (b["aug"][:, 5] == 7).all()
    # the same call again: the same batch; another step: another one
    again = batch_of(s)
    assert all(torch.equal(b[k], again[k]) for k in b)
    assert not torch.equal(batch_of(s, object_offset=2)["ref_rotation"], b["ref_rotation"])
    # rendered at the jittered pose under the adapted intrinsics
    img, depth, _ = r.render(b["ref_rotation"], b["ref_translation"], b["internel_k"], b["label"])
    assert torch.equal(b["render_images"], img) and torch.equal(b["depth"], depth)
    assert (depth > 0).float().mean() > 0.1
    # internel_k projects the model points where T maps their frame projections
    points, counts = patches.point_table(r.renderer)
    T, k, K = (x.double().cpu().numpy() for x in (b["transform_matrix"], b["internel_k"], s["ori_k"]))
    for i in range(2):
        lab = int(s["labels"][i])
        X = points[lab, :int(counts[lab])].double().cpu().numpy()
        cam = X @ b["ref_rotation"][i].double().cpu().numpy().T + b["ref_translation"][i].double().cpu().numpy()
        pf, pp = cam @ K[i].T, cam @ k[i].T
        pf, pp = pf / pf[:, 2:], pp[:, :2] / pp[:, 2:]
        err = np.abs((pf @ T[i].T)[:, :2] - pp).max()
        print(f"object {i}: geom {b['geom'][i].tolist()}, max |k·X − T·K·X| {err:.2e} px")
        assert err <= 1e-3
        assert pp.min() >= 0 and pp.max() <= S - 1  # the crop at the jittered pose holds its points
    # drop_invalid keeps the valid objects (all, here) in order
    c = batch_of(s, drop_invalid=True)
    assert all(torch.equal(b[k], c[k]) for k in b)
    pts = [p.cuda() for p in torch.from_numpy(synthetic.make_model_points(256)).float()]
    step = TrainStep(r, pts, list(synthetic.YCBV_DIAMETERS))
    out = step({k: b[k] for k in ("real_images", "render_images", "depth", "internel_k", "ref_rotation",
                                  "ref_translation", "gt_rotation", "gt_translation", "label",
                                  "gt_masks")})
    loss = float(out["loss"].detach())
    print("loss", loss)
    assert np.isfinite(loss) and loss > 0
