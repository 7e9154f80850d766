"""GPU: ``patches.frames_to_patches`` and ``SCFlowRefiner.refine_frames`` on synthetic 300×400
frames — 256² renders of the synthetic scene pasted at known offsets, the camera matrix shifted by
the same offsets — so a decoded frame plus detections goes to refined poses in one call."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import patch_restatement as pr

pytest.importorskip("oracle.scflow_oracle")
pytestmark = pytest.mark.gpu

S, FH, FW = 256, 300, 400
OFFSETS = [(100, 30), (20, 44)]  # (x, y) of each render's top-left corner in its frame


@lru_cache(maxsize=None)
def setup():
    from scflow_amd import MODELS, synthetic
    from tests.helpers import refiner_state_dict
    from tests.test_gpu_decoder import decoder_cfg
    sc = synthetic.make_scene(2, S, seed=21)
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
                          test_cfg=dict(iters=2, cycles=1)))
    r.load_state_dict({("decoder." + k if not k.startswith(("real_encoder.", "render_encoder.", "context."))
                        else k): v for k, v in refiner_state_dict().items()}, strict=False)
    r = r.eval().cuda()
    R, t, K, lab = (torch.from_numpy(sc[k]).cuda() for k in ("ref_rotation", "ref_translation",
                                                             "internel_k", "labels"))
    tgt = synthetic.make_train_targets(sc, S, seed=21)
    real, _, _ = r.render(torch.from_numpy(tgt["gt_rotation"]).cuda(),
                          torch.from_numpy(tgt["gt_translation"]).cuda(), K, lab)
    # frames as a decoder delivers them: uint8, interleaved, BGR
    bgr = (real.flip(1) * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    frames = torch.full((2, FH, FW, 3), 128, dtype=torch.uint8, device="cuda")
    ori_k = K.clone()
    for i, (ox, oy) in enumerate(OFFSETS):
        frames[i, oy:oy + S, ox:ox + S] = bgr[i]
        ori_k[i, 0, 2] += ox
        ori_k[i, 1, 2] += oy
    return dict(refiner=r, R=R, t=t, K=K, labels=lab, frames=frames.contiguous(), ori_k=ori_k,
                fidx=torch.arange(2, device="cuda"))


def test_frames_to_patches_keeps_the_projection():
    from scflow_amd import patches
    s = setup()
    points, counts = patches.point_table(s["refiner"].renderer)
    data = patches.frames_to_patches(s["frames"], s["fidx"], s["R"], s["t"], s["ori_k"], s["labels"],
                                     points, counts, size=S)
    assert set(data) >= {"real_images", "internel_k", "transform_matrix", "ori_k", "valid", "crop_boxes"}
    assert tuple(data["real_images"].shape) == (2, 3, S, S) and data["valid"].tolist() == [True, True]
    assert torch.equal(data["ori_k"], s["ori_k"]) and tuple(data["crop_boxes"].shape) == (2, 4)
    T, k, K = (data[n].double().cpu().numpy() for n in ("transform_matrix", "internel_k", "ori_k"))
    for i in range(2):
        lab = int(s["labels"][i])
        X = points[lab, :int(counts[lab])].double().cpu().numpy()
        cam = X @ s["R"][i].double().cpu().numpy().T + s["t"][i].double().cpu().numpy()
        pf, pp = cam @ K[i].T, cam @ k[i].T
        pf, pp = pf / pf[:, 2:], pp[:, :2] / pp[:, 2:]
        err = np.abs((pf @ T[i].T)[:, :2] - pp).max()
        print(f"object {i}: crop {data['crop_boxes'][i].tolist()}, max |k·X − T·K·X| {err:.2e} px")
        assert err <= 1e-3
        # the ratio-1.1 crop holds every projected point, and the object fills most of the patch
        assert pp.min() >= 0 and pp.max() <= S - 1 and np.ptp(pp, 0).max() >= 0.85 * S
    # the same patches as the restatement, stage by stage, at 256² (64 bands of 4 rows per patch)
    geom, fidx = data["geom"].cpu().numpy(), s["fidx"].cpu().numpy()
    want = pr.extract_all(s["frames"].cpu().numpy(), fidx, geom, [1, 1], S, dtype=np.float64,
                          pad=128.0, std=[255.0] * 3, to_rgb=True, quantize=False)
    scaled = data["real_images"].double().cpu().numpy() * 255  # std 255: levels / 255 in fp32
    got = np.rint(scaled)
    assert np.abs(scaled - got).max() <= 1e-4
    want_q = np.rint(want * 255)
    clear = np.abs(want * 255 - np.floor(want * 255) - 0.5) > 1e-3
    assert np.abs(got - want_q).max() <= 1 and np.array_equal(got[clear], want_q[clear])
    # a map under the same geometry: the mask of the frame's non-background pixels
    mask = (s["frames"] != 128).any(-1, keepdim=True).to(torch.uint8).contiguous()
    m = patches.extract_maps(mask, s["fidx"], data["geom"], data["valid"], S, mode="nearest")
    want_m = pr.extract_all(mask.cpu().numpy(), fidx, geom, [1, 1], S, dtype=np.float32, pad=0.0,
                            nearest=True)
    assert tuple(m.shape) == (2, 1, S, S) and np.array_equal(m.cpu().numpy(), want_m)
    assert 0.2 < float(m.mean()) < 0.9


def test_refine_frames_is_refine_on_the_patches():
    from scflow_amd import patches
    s = setup()
    r = s["refiner"]
    cat = lambda x, y: torch.cat([x, y[:1]])  # noqa: E731
    R, t, lab = cat(s["R"], s["R"]), cat(s["t"], s["t"]), cat(s["labels"], s["labels"])
    ori_k = cat(s["ori_k"], s["ori_k"])
    fidx = torch.tensor([0, 1, -1], device="cuda")  # the third detection names no frame
    Ro, to, valid, data = r.refine_frames(s["frames"], fidx, R, t, ori_k, lab, cycles=1)
    assert valid.tolist() == [True, True, False]
    points, counts = patches.point_table(r.renderer)
    d2 = patches.frames_to_patches(s["frames"], fidx, R, t, ori_k, lab, points, counts, size=S)
    for key in ("real_images", "internel_k", "transform_matrix"):
        assert torch.equal(d2[key], data[key])
    R2, t2, _ = r.refine(d2["real_images"], R, t, d2["internel_k"], lab, cycles=1)
    assert torch.equal(Ro[:2], R2[:2]) and torch.equal(to[:2], t2[:2])
    assert torch.equal(Ro[2], R[2]) and torch.equal(to[2], t[2])  # untouched
    assert not torch.equal(Ro[:2], R[:2]) and torch.isfinite(Ro).all() and torch.isfinite(to).all()
    assert (d2["real_images"][2] == torch.tensor(128.0) / 255).all()
    assert torch.equal(d2["internel_k"][2], ori_k[2])
