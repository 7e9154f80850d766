"""GPU: ``patches.frames_to_train_patches`` and ``SCFlowRefiner.train_batch_from_frames`` with a
background pool, on the synthetic frames of tests/test_gpu_train_patch_refiner.py:
without a pool today's batch, with one the composite — and a ``TrainStep`` on it."""
import numpy as np
import pytest
import torch

pytest.importorskip("oracle.scflow_oracle")
pytestmark = pytest.mark.gpu

from tests.test_gpu_train_patch_refiner import S, SEED, STEP, batch_of, setup  # noqa: E402


def _pool():
    from scflow_amd import synthetic
    pool, sizes = synthetic.make_background_pool(4, 60, 80, seed=3)
    return torch.from_numpy(pool).cuda(), torch.from_numpy(sizes).cuda()


def _patches(s, **kw):
    from scflow_amd import patches
    points, counts = patches.point_table(s["refiner"].renderer)
    return patches.frames_to_train_patches(s["frames"], s["masks"], s["fidx"], s["Rg"], s["tg"],
                                           s["ori_k"], s["labels"], points, counts, s["diam"], SEED,
                                           STEP, size=S, **kw)


def test_frames_to_train_patches_with_and_without_a_pool():
    from scflow_amd import ops
    s = setup()
    pool, sizes = _pool()
    plain = _patches(s)
    assert "background_index" not in plain
    none = _patches(s, backgrounds=pool, background_sizes=sizes, background_p=0.0)
    assert none["background_index"].tolist() == [-1, -1] and none["background_index"].dtype == torch.int32
    for k in plain:
        assert torch.equal(plain[k], none[k]), k
    index = torch.tensor([2, -1], device="cuda")
    got = _patches(s, backgrounds=pool, background_sizes=sizes, background_index=index)
    assert got["background_index"].tolist() == [2, -1]
    for k in plain:
        if k != "real_images":
            assert torch.equal(plain[k], got[k]), k
    assert torch.equal(got["real_images"][1], plain["real_images"][1])
    # the object keeps its pixels, its surroundings (the frames' flat 128 and the pad) do not
    fg = plain["gt_masks"][0] > 0
    changed = (got["real_images"][0] != plain["real_images"][0]).any(0)
    print(f"object 0: {changed[~fg].float().mean():.1%} of the background and "
          f"{changed[fg].float().mean():.1%} of the foreground pixels of the patch changed")
    assert changed[~fg].float().mean() > 0.9 and changed[fg].float().mean() < 0.2
    # what the op gives under the batch's own geometry and rows
    want, _ = ops.extract_patches_aug_bg(
        s["frames"], s["masks"], s["fidx"].to(torch.int32), got["geom"], got["valid"].to(torch.uint8),
        got["aug"], pool, S, SEED, STEP, background_sizes=sizes,
        background_index=index.to(torch.int32), mean=[0.0] * 3, std=[255.0] * 3, to_rgb=True)
    assert torch.equal(got["real_images"], want)
    # drawn: a function of (seed, step, object_offset + i) alone
    from tests import train_patch_bg_restatement as bg
    drawn = _patches(s, backgrounds=pool, background_sizes=sizes, background_p=0.5, object_offset=6)
    assert drawn["background_index"].tolist() == [bg.draw(6 + i, SEED, STEP, 0.5, 4) for i in range(2)]


def test_train_step_on_a_batch_with_backgrounds():
    from scflow_amd import synthetic
    from scflow_amd.train.step import TrainStep
    s = setup()
    r = s["refiner"]
    pool, sizes = _pool()
    b = batch_of(s, backgrounds=pool, background_sizes=sizes, background_p=1.0)
    plain = batch_of(s)
    assert (b["background_index"] >= 0).all() and b["valid"].all()
    assert not torch.equal(b["real_images"], plain["real_images"])
    for k in ("render_images", "depth", "ref_rotation", "internel_k", "gt_masks"):
        assert torch.equal(b[k], plain[k]), k
    c = batch_of(s, backgrounds=pool, background_sizes=sizes, background_p=1.0, drop_invalid=True)
    assert all(torch.equal(b[k], c[k]) for k in b)
    pts = [p.cuda() for p in torch.from_numpy(synthetic.make_model_points(256)).float()]
    step = TrainStep(r, pts, list(synthetic.YCBV_DIAMETERS))
    out = step({k: b[k] for k in ("real_images", "render_images", "depth", "internel_k", "ref_rotation",
                                  "ref_translation", "gt_rotation", "gt_translation", "label",
                                  "gt_masks")})
    loss = float(out["loss"].detach())
    print("loss", loss)
    assert np.isfinite(loss) and loss > 0
