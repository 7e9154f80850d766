"""GPU: scflow_train_draw / scflow_train_patch_extract (``ops.train_draw``,
``ops.extract_patches_aug``) against the NumPy restatement of the contract
(tests/train_patch_restatement.py).

Shapes are those of tests/test_gpu_patch_ops.py — F = 2 frames of 48×64, S = 32, geometry and aug
rows given directly.  Bounds:

* stage mask 0: ``ops.extract_patches``' bits;
* HSV and blur: integer levels equal to the fp32 restatement, within one level of the fp64 one.
  The two-sided comparison uses gains with a short mantissa: the contract truncates level · gain
  after ONE fp32 rounding, so with gains such as 1.15 the fp32 product can reach an integer the
  fp64 product stays below — a whole H unit (2°), up to 5 levels on about 2 % of the pixels of
  these crops, measured with the two restatements alone.  Such gains are compared with the fp32
  restatement only;
* noise: the device's logf / cosf / sinf are not NumPy's, so levels are compared with the fp64
  restatement wherever its value before truncation lies more than 1e-3 from an integer (the
  precise libm calls keep the device within about 3e-5 levels: |z| ≤ 6 carries a few ulp, times
  sigma·255 ≤ 26), and within one level elsewhere; at most 1 % of the values may be that close
  (expected 0.2 %);
* the whole chain: exact, by reading the device's own HSV + noise crop at identity geometry and
  restating the blur and the resize on it;
* ``train_draw``: words, ratio and aug rows exact; R_ref within 2e-6 and t_ref within 2e-6·max(1,
  ‖t‖) of the fp64 restatement; ``ok`` / ``tries`` its decisions, on seeds for which every fp64
  margin to a limit exceeds 1e-3 relative (asserted).
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import patch_restatement as pr
from tests import train_patch_restatement as tr
from tests.test_gpu_patch_ops import (BOXES, FRAME_INDEX, H, MEAN, PAD, RGB, S, STD, VALID, W,
                                      _wide_case, case, dev, gpu)

pytestmark = pytest.mark.gpu

SEED, STEP = 0x5CF10A3D2B17, 5
HSV, NOISE, BLUR = tr.AUG_HSV, tr.AUG_NOISE, tr.AUG_BLUR
AUG_BOXES = [(10, 5, 29, 24),      # inside the frame (crop 20)
             (-7, -5, 13, 14),     # leaves it top-left (21 × 20)
             (40, 25, 80, 64),     # leaves it bottom-right (41 × 40)
             (-10, -20, 79, 69),   # larger than the frame (crop 90)
             (20, 10, 21, 30)]     # two pixels wide: the blur folds −2 … 3 onto 0, 1
AUG_FIDX = [0, 1, 0, 1, 1]
# gains with a short mantissa: level · gain is exact in fp32 and in fp64, so both truncate alike
GAINS = [(1.125, 0.75, 1.25), (0.875, 1.375, 0.625), (1.0, 1.0, 1.0), (1.1875, 1.5, 1.5),
         (0.8125, 0.5, 0.875)]
# any gains: the fp32 product may round up to the integer that the fp64 product stays below
ANY_GAINS = [(1.15, 0.7, 1.3), (0.85, 1.4, 0.6), (1.07, 1.0, 0.93), (1.2, 1.5, 1.5), (0.8, 0.5, 0.9)]


def rows_of(mask, ksize=1, sigma=0.07, n=len(AUG_BOXES), gains=GAINS):
    return np.array([gains[i % len(gains)] + (sigma, ksize, mask, 0, 0) for i in range(n)],
                    np.float32)


def extract(frames, fidx, geom, rows, size=S, valid=None, **kw):
    from scflow_amd import ops
    n = len(geom)
    valid = [1] * n if valid is None else valid
    kw.setdefault("seed", SEED), kw.setdefault("step", STEP)
    frames = frames if isinstance(frames, torch.Tensor) else dev(frames)
    return ops.extract_patches_aug(frames, dev(fidx, torch.int32), dev(np.asarray(geom, np.int32)),
                                   dev(valid, torch.uint8), dev(rows), size, **kw)


def levels(t):
    a = t.cpu().numpy()
    assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= 255
    return a


def restate(frames, fidx, geom, rows, dtype, size=S, offset=0):
    return np.stack([tr.extract_aug(frames[f], g, r, offset + i, size, SEED, STEP, dtype)
                     for i, (f, g, r) in enumerate(zip(fidx, geom, rows))])


# ------------------------------------------------------------------------------ extract
def test_stage_mask_zero_is_extract_patches():
    from scflow_amd import ops
    g = gpu()
    n = len(BOXES)
    rows = dev(rows_of(0, ksize=5, n=n))
    for quantize in (True, False):
        want = ops.extract_patches(g["frames"], g["fidx"], g["geom"], g["valid"], S,
                                   quantize=quantize, **RGB)
        for direct in (False, True):
            got = ops.extract_patches_aug(g["frames"], g["fidx"], g["geom"], g["valid"], rows, S,
                                          SEED, STEP, pad=int(PAD), mean=MEAN, std=STD, to_rgb=True,
                                          quantize=quantize, direct=direct)
            assert torch.equal(got, want)
    assert want[:6].std() > 0


@pytest.mark.parametrize("mask,ksize", [(HSV, 1), (BLUR, 3), (BLUR, 5), (HSV | BLUR, 3),
                                        (HSV | BLUR, 5)])
def test_hsv_and_blur_equal_the_fp32_restatement(mask, ksize):
    frames = case()["frames"]
    geom = [pr.geom_of(*b, S) for b in AUG_BOXES]
    assert geom[4][4:6] == (3, 32)
    rows = rows_of(mask, ksize)
    got = levels(extract(frames, AUG_FIDX, geom, rows))
    assert np.array_equal(got, levels(extract(frames, AUG_FIDX, geom, rows, direct=True)))
    want32 = restate(frames, AUG_FIDX, geom, rows, np.float32)
    want64 = restate(frames, AUG_FIDX, geom, rows, np.float64)
    plain = restate(frames, AUG_FIDX, geom, rows_of(0), np.float32)
    assert not np.array_equal(want32, plain)  # the stage does something
    print(f"mask {mask} k {ksize}: {(got != want64).mean():.4%} of the levels differ from the fp64 "
          f"restatement, {(got != want32).sum()} from the fp32 one")
    assert np.array_equal(got, want32)
    assert np.abs(got - want64).max() <= 1
    if mask & HSV:  # gains as they are drawn: the fp32 definition holds; fp64 truncates elsewhere
        rows = rows_of(mask, ksize, gains=ANY_GAINS)
        got = levels(extract(frames, AUG_FIDX, geom, rows))
        assert np.array_equal(got, restate(frames, AUG_FIDX, geom, rows, np.float32))
        d = np.abs(got - restate(frames, AUG_FIDX, geom, rows, np.float64))
        print(f"  any gains: {(d > 0).mean():.3%} differ from the fp64 restatement, by up to {d.max():.0f}")


def _identity(box):
    """A square crop at S = its side: nw = nh = S, no padding, every output pixel IS a crop pixel."""
    side = box[2] - box[0] + 1
    assert side == box[3] - box[1] + 1 and side % 4 == 0
    g = pr.geom_of(*box, side)
    assert g[4:] == (side, side, 0, 0)
    return side, g


@pytest.mark.parametrize("box,fi", [((10, 5, 29, 24), 0), ((-7, -5, 12, 14), 1), ((8, 1, 51, 44), 1)])
def test_noise_at_identity_geometry(box, fi):
    frames = case()["frames"]
    side, g = _identity(box)
    row = rows_of(NOISE, sigma=0.1, n=1)
    got = levels(extract(frames, [fi], [g], row, size=side, object_offset=3))[0]  # [3, side, side]
    crop = pr.crop(frames[fi], *box, 128, np.uint8)
    exact = tr.noise_values(crop, 0.1, 3, SEED, STEP, np.float64).transpose(2, 0, 1)
    want = np.clip(exact, 0, 255).astype(np.uint8)
    near = (np.abs(exact - np.rint(exact)) <= 1e-3) & (exact > -1e-3) & (exact < 255 + 1e-3)
    print(f"crop {side}: {near.mean():.3%} of the values within 1e-3 of an integer, "
          f"{(got != want).sum()} levels differ, clipped {((exact < 0) | (exact > 255)).mean():.2%}")
    assert near.mean() <= 0.01
    assert np.array_equal(got[~near], want[~near]) and np.abs(got - want).max() <= 1
    assert (got != crop.transpose(2, 0, 1)).mean() > 0.9


def test_full_chain_is_exact_on_the_devices_own_augmented_crop():
    """HSV + noise read back at identity geometry, then blur and resize restated: the S = 32 output
    of the same objects, bit for bit — so the noise a crop pixel gets depends neither on S nor on
    the tiling, and the blur and the resize see exactly that crop."""
    frames = case()["frames"]
    boxes, fidx = [(10, 5, 29, 24), (8, 1, 51, 44), (30, 20, 45, 35)], [0, 1, 0]
    for ksize in (3, 5):
        rows = rows_of(HSV | NOISE | BLUR, ksize, n=3)
        geom = [pr.geom_of(*b, S) for b in boxes]
        full = levels(extract(frames, fidx, geom, rows))
        assert np.array_equal(full, levels(extract(frames, fidx, geom, rows, direct=True)))
        for i, b in enumerate(boxes):
            side, g = _identity(b)
            pre = rows[i:i + 1].copy()
            pre[0, 5] = HSV | NOISE
            own = levels(extract(frames, fidx[i:i + 1], [g], pre, size=side, object_offset=i))[0]
            crop = own.transpose(1, 2, 0).astype(np.uint8)
            want = tr.finish(tr.blur_stage(crop, ksize), geom[i], S)
            assert np.array_equal(full[i], want), (ksize, i)


def test_routes_give_the_same_bits_on_a_crop_wider_than_the_window():
    """A 4000 × 200 crop of a 16 × 4096 frame has no band whose rows fit the LDS window: every tap
    computes its own; the 60-wide crop next to it is staged."""
    frames, geom = _wide_case()
    rows = rows_of(HSV | BLUR, 5, n=2)
    got = levels(extract(frames, [0, 0], geom, rows))
    assert np.array_equal(got, levels(extract(frames, [0, 0], geom, rows, direct=True)))
    assert np.array_equal(got, restate(frames, [0, 0], geom, rows, np.float32))
    rows[:, 5] = HSV | NOISE | BLUR
    noisy = extract(frames, [0, 0], geom, rows)
    assert torch.equal(noisy, extract(frames, [0, 0], geom, rows, direct=True))
    assert not np.array_equal(levels(noisy), got)


def test_patch_sides_with_several_column_tiles():
    """S = 96: a workgroup's tile is 16 × 64 output pixels, so a patch row is cut at column 64
    (tiles of 64 and 32 columns, six bands); S = 32 is one tile."""
    frames = case()["frames"]
    geom = [pr.geom_of(*b, 96) for b in AUG_BOXES]
    rows = rows_of(HSV | BLUR, 5)
    got = levels(extract(frames, AUG_FIDX, geom, rows, size=96))
    assert np.array_equal(got, levels(extract(frames, AUG_FIDX, geom, rows, size=96, direct=True)))
    assert np.array_equal(got, restate(frames, AUG_FIDX, geom, rows, np.float32, size=96))
    rows[:, 5] = HSV | NOISE | BLUR
    noisy = extract(frames, AUG_FIDX, geom, rows, size=96)
    assert torch.equal(noisy, extract(frames, AUG_FIDX, geom, rows, size=96, direct=True))
    assert not np.array_equal(levels(noisy), got)


def _flat(**kw):
    """Noise only on a constant-128 frame at identity geometry: [3, 64, 64] levels."""
    frames = np.full((1, 64, 64, 3), 128, np.uint8)
    out = extract(frames, [0], [pr.geom_of(0, 0, 63, 63, 64)], rows_of(NOISE, sigma=0.1, n=1),
                  size=64, **kw)
    return levels(out)[0].astype(np.float64)


def test_noise_keying_and_statistics():
    a = _flat()
    assert np.array_equal(a, _flat()) and np.array_equal(a, _flat(direct=True))
    n = a[0].size
    rho = lambda x, y: abs(np.corrcoef(x.ravel(), y.ravel())[0, 1])  # noqa: E731
    others = dict(step=_flat(step=STEP + 1), offset=_flat(object_offset=1), seed=_flat(seed=SEED + 1))
    for name, b in others.items():
        print(f"{name}: |rho| = {rho(a, b):.4f} (bound {4 / np.sqrt(3 * n):.4f})")
        assert rho(a, b) < 4 / np.sqrt(3 * n)
    for c, d in ((0, 1), (0, 2), (1, 2)):
        assert rho(a[c], a[d]) < 4 / np.sqrt(n)
    # truncation lowers the mean by half a level; four standard errors of 12 288 samples
    print(f"mean {a.mean():.3f}, std {a.std():.3f}")
    assert abs(a.mean() - 127.5) <= 0.92 and abs(a.std() - 25.5) <= 0.65


# ------------------------------------------------------------------------------ draw
N_DRAW, DRAW_SEED, DRAW_STEP, DRAW_OFFSET = 64, 77, 2, 5
DIAMETERS = [170.0, 150.0, 200.0]
CONFIGS = dict(
    config={},                                                       # the config's limits
    angle10=dict(angle_limit=10.0),                                  # many rejections
    add=dict(angle_limit=-1.0, translation_limit=-1.0, add_limit=0.2),  # the reduction decides
    hopeless=dict(angle_limit=0.01),                                 # tries run out
    off=dict(angle_limit=-1.0, translation_limit=-1.0, add_limit=-1.0),
    other=dict(angle_mean=3.0, angle_std=5.0, x_mean=-4.0, z_mean=20.0, ratio_lo=1.1,
               ratio_hi=1.4, noise_ratio=0.3, max_kernel_size=3, p_hsv=0.5, p_noise=0.3,
               p_blur=0.7))
MAX_TRIES = dict(hopeless=6)


@lru_cache(maxsize=None)
def draw_inputs():
    rng = np.random.default_rng(7)
    points = rng.uniform(-60.0, 60.0, (3, 64, 3)).astype(np.float32)
    counts = np.array([64, 40, 64], np.int32)
    labels = rng.integers(0, 3, N_DRAW).astype(np.int32)
    Rs, ts = [], []
    for _ in range(N_DRAW):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        Rs.append((q * np.sign(np.linalg.det(q))).astype(np.float32))
        tz = rng.uniform(500.0, 1500.0)
        ts.append(np.array([rng.uniform(-0.3, 0.3) * tz, rng.uniform(-0.2, 0.2) * tz, tz], np.float32))
    return points, counts, labels, np.stack(Rs), np.stack(ts)


@lru_cache(maxsize=None)
def draw_restated(name):
    points, counts, labels, R, t = draw_inputs()
    cfg = dict(tr.CFG, **CONFIGS[name])
    out = [tr.draw(points[l, :counts[l]], DIAMETERS[l], R[i], t[i], DRAW_OFFSET + i, DRAW_SEED,
                   DRAW_STEP, cfg, MAX_TRIES.get(name, 32)) for i, l in enumerate(labels)]
    margin = min((m for o in out for m in o["margins"]), default=1.0)
    assert margin > 1e-3, f"{name}: a decision lies {margin:.2e} (relative) from its limit"
    return cfg, out


def run_draw(name, sl=slice(None), offset=DRAW_OFFSET, counts=None, labels=None):
    from scflow_amd import ops
    points, cnt, lab, R, t = draw_inputs()
    cnt = cnt if counts is None else counts
    lab = (lab if labels is None else labels)[sl]
    cfg = dict(tr.CFG, **CONFIGS[name])
    out = ops.train_draw(dev(points), dev(cnt), dev(lab), dev(DIAMETERS, torch.float32), dev(R[sl]),
                         dev(t[sl]), cfg, DRAW_SEED, DRAW_STEP, offset, MAX_TRIES.get(name, 32))
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_train_draw_matches_the_restatement(name):
    cfg, want = draw_restated(name)
    R, t, err, ok, tries, ratio, aug = run_draw(name)
    _, _, _, Rg, tg = draw_inputs()
    for i, w in enumerate(want):
        wr, wrow = tr.aug_row(DRAW_OFFSET + i, DRAW_SEED, DRAW_STEP, cfg)
        assert ratio[i] == wr and np.array_equal(aug[i], wrow), i
        assert (int(ok[i]), int(tries[i])) == (w["ok"], w["tries"]), i
        assert np.abs(R[i] - w["R"]).max() <= 2e-6, i
        # t = t_gt + Δt is a sum of terms of either sign: its error scales with the vector's
        # magnitude (‖t‖ ≥ 500 here, |Δt| ≤ 200), not with a component that nearly cancels
        assert np.abs(t[i] - w["t"]).max() <= 2e-6 * max(1.0, np.linalg.norm(w["t"])), i
        # add and ‖Δt‖ carry a few ulp of coordinates ~1e3 relative to distances ~1e1; the angle
        # comes through acos, whose error is the trace's (≤ 1e-6) over sin(angle)
        assert abs(err[i, 0] - w["add"]) <= 1e-4 * max(w["add"], 1e-2), i
        assert abs(err[i, 2] - w["trans"]) <= 1e-5 * max(w["trans"], 1.0), i
        tol = np.degrees(1e-6 / max(np.sin(np.radians(w["rot"])), 1e-3))
        assert abs(err[i, 1] - w["rot"]) <= tol, i
        if not w["ok"]:
            assert np.array_equal(R[i], Rg[i]) and np.array_equal(t[i], tg[i]) and not err[i].any()
    mean_tries = tries.mean()
    print(f"{name}: {int(ok.sum())} of {N_DRAW} accepted, {mean_tries:.2f} tries on average, "
          f"max {tries.max()}")
    if name == "config":
        assert ok.all() and tries.max() <= 8
        assert (err[:, 1] <= 45).all() and (err[:, 2] <= 200).all() and (err[:, 0] <= 1).all()
        assert set(aug[:, 4]) == {1.0, 3.0, 5.0} and (aug[:, 5] == 7).all()
    if name == "angle10":
        assert ok.sum() >= N_DRAW // 2 and (tries > 1).sum() >= N_DRAW // 2 and (err[ok != 0, 1] <= 10).all()
    if name == "add":
        assert (tries > 1).any() and (err[ok != 0, 0] <= 0.2).all()
    if name == "hopeless":
        assert not ok.any() and (tries == 6).all()
    if name == "off":
        assert ok.all() and (tries == 1).all()
    if name == "other":
        assert set(aug[:, 4]) == {1.0, 3.0} and len(set(aug[:, 5])) >= 4
        assert ((ratio >= np.float32(1.1)) & (ratio < np.float32(1.4))).all()


def test_train_draw_object_offset_and_ragged_tables():
    full = run_draw("config")
    k = 9
    part = run_draw("config", slice(k, None), DRAW_OFFSET + k)
    for a, b in zip(full, part):
        assert np.array_equal(a[k:], b)
    # a class without points and a label outside the table: no ADD, a pose all the same; the box
    # kernel then makes them invalid
    from scflow_amd import ops
    points, counts, labels, Rg, tg = draw_inputs()
    labels = labels.copy()
    labels[:4] = [2, 2, 7, -1]
    R, t, err, ok, tries, ratio, aug = run_draw("config", counts=np.array([64, 40, 0], np.int32),
                                                labels=labels)
    assert ok[:4].all() and not err[:4, 0].any() and (err[:4, 2] > 0).all()
    K = np.repeat(np.array([[[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]]], np.float32), N_DRAW, 0)
    valid = ops.patch_boxes(dev(points), dev(np.array([64, 40, 0], np.int32)), dev(labels), dev(R),
                            dev(t), dev(K), dev(ratio), 480, 640, S)[4].cpu().numpy()
    assert not valid[:4].any() and valid[labels < 2].any()


# ------------------------------------------------------------------------------ plumbing
def _pipeline():
    """Draw, boxes and the augmented extract back to back on two 480 × 640 frames."""
    from scflow_amd import ops
    points, counts, labels, R, t = draw_inputs()
    n = 8
    frames = dev(np.random.default_rng(2).integers(0, 256, (2, 480, 640, 3), dtype=np.uint8))
    K = dev(np.array([[[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]],
                      [[1066.8, 0, 312.99], [0, 1067.5, 241.3], [0, 0, 1]]], np.float32))
    fidx = dev(np.arange(n) % 2, torch.int32)
    args = (dev(points), dev(counts), dev(labels[:n]), dev(DIAMETERS, torch.float32), dev(R[:n]),
            dev(t[:n]))

    def go():
        Rr, tr_, err, ok, tries, ratio, aug = ops.train_draw(*args, tr.CFG, DRAW_SEED, DRAW_STEP)
        bbox, geom, T, k, valid = ops.patch_boxes(args[0], args[1], args[2], Rr, tr_, K, ratio, 480,
                                                  640, S, frame_index=fidx, num_frames=2,
                                                  k_per_frame=True)
        img = ops.extract_patches_aug(frames, fidx, geom, valid, aug, S, DRAW_SEED, DRAW_STEP,
                                      mean=MEAN, std=STD, to_rgb=True)
        return Rr, tr_, err, ok, tries, ratio, aug, geom, k, valid, img
    return go


def test_runs_on_the_current_stream():
    go = _pipeline()
    want = go()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = go()  # no synchronisation between the three launches
    s.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert want[9].any() and want[10].std() > 0


def test_graph_capture_and_replay():
    go = _pipeline()
    eager = go()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        go()  # allocator warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):  # one chain: draw → boxes → extract
        out = go()
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)


def test_no_objects_and_refusals():
    from scflow_amd import ops
    from scflow_amd._lib import ScflowError
    g = gpu()
    points, counts, _, _, _ = draw_inputs()
    e = lambda *s, dt=torch.float32: torch.empty(*s, device="cuda", dtype=dt)  # noqa: E731
    out = ops.train_draw(dev(points), dev(counts), e(0, dt=torch.int32), dev(DIAMETERS, torch.float32),
                         e(0, 3, 3), e(0, 3), tr.CFG, 1, 0)
    assert [tuple(o.shape) for o in out] == [(0, 3, 3), (0, 3), (0, 3), (0,), (0,), (0,), (0, 8)]
    img = ops.extract_patches_aug(g["frames"], e(0, dt=torch.int32), e(0, 8, dt=torch.int32),
                                  e(0, dt=torch.uint8), out[6], S, 1, 0)
    assert tuple(img.shape) == (0, 3, S, S)
    rows = dev(rows_of(0, n=len(BOXES)))
    with pytest.raises(ScflowError, match="pad"):
        ops.extract_patches_aug(g["frames"], g["fidx"], g["geom"], g["valid"], rows, S, 1, 0, pad=127.5)
    with pytest.raises(ScflowError, match=r"\[8, 8\]"):
        ops.extract_patches_aug(g["frames"], g["fidx"], g["geom"], g["valid"], rows[:, :6].contiguous(),
                                S, 1, 0)
    with pytest.raises(ScflowError, match="uint8"):
        ops.extract_patches_aug(g["depth"], g["fidx"], g["geom"], g["valid"], rows, S, 1, 0)
    with pytest.raises(ScflowError, match="cfg lacks"):
        ops.train_draw(dev(points), dev(counts), dev([0], torch.int32), dev(DIAMETERS, torch.float32),
                       e(1, 3, 3), e(1, 3), dict(angle_mean=0.0), 1, 0)
    # rows that are no aug rows switch the stages off instead of indexing anything with them
    bad = rows.clone()
    bad[:, 4], bad[:, 5] = float("nan"), float("nan")
    bad[1, 5], bad[2, 5], bad[3, 4], bad[3, 5] = 99.0, -3.0, 4.0, 4.0
    want = ops.extract_patches(g["frames"], g["fidx"], g["geom"], g["valid"], S)
    assert torch.equal(ops.extract_patches_aug(g["frames"], g["fidx"], g["geom"], g["valid"], bad, S,
                                               1, 0), want)


def test_opcheck_train_patch_ops():
    from scflow_amd import library  # noqa: F401  (registers the ops)
    from scflow_amd._lib import TRAIN_CFG
    g = gpu()
    points, counts, labels, R, t = draw_inputs()
    cfg = [float(tr.CFG[k]) for k in TRAIN_CFG]
    args = (dev(points), dev(counts), dev(labels[:4]), dev(DIAMETERS, torch.float32), dev(R[:4]),
            dev(t[:4]), cfg, 5, 32, DRAW_SEED, DRAW_STEP, DRAW_OFFSET)
    torch.library.opcheck(torch.ops.scflow.train_draw.default, args)
    got = torch.ops.scflow.train_draw(*args)
    for a, b in zip(got, run_draw("config", slice(0, 4))):
        assert np.array_equal(a.cpu().numpy(), b)
    rows = dev(rows_of(HSV | NOISE | BLUR, 3, n=len(BOXES)))
    eargs = (g["frames"], g["fidx"], g["geom"], g["valid"], rows, S, SEED, STEP, 0, int(PAD), MEAN,
             STD, True, True)
    torch.library.opcheck(torch.ops.scflow.patch_extract_aug.default, eargs)
    want = extract(g["frames"], FRAME_INDEX, case()["geom"], rows_of(HSV | NOISE | BLUR, 3, n=len(BOXES)),
                   valid=VALID, pad=int(PAD), mean=MEAN, std=STD, to_rgb=True)
    assert torch.equal(torch.ops.scflow.patch_extract_aug(*eargs), want)
    assert H == 48 and W == 64
