"""GPU: scflow_patch_boxes / scflow_patch_extract (``ops.patch_boxes``, ``ops.extract_patches``)
against the NumPy restatement of the contract (tests/patch_restatement.py).

Shapes are small — F = 2 frames of 48×64, S = 32 (one workgroup per patch), eight objects whose
geometry is given directly — and cover: up- and downscale, an exact 2×, crops leaving the frame on
either side and larger than it, a non-square crop with odd padding, an invalid object and a frame
index outside the frames.  Bounds:

* unquantised bilinear against the fp64 restatement: |error| ≤ 2e-6·(255/std).  About ten fp32
  roundings on values ≤ 255 give ≤ 1.5e-4 levels, 6e-7 after /255; the bound is three times that;
* the exact 2× crop, padding, invalid patches, channel order, nearest: equality;
* quantised: integer levels, within one level of the fp64 restatement, equal wherever the fp64
  value lies more than 1e-3 from a half-integer;
* LDS-staged and direct routes: the same bits;
* ``patch_boxes``: ``geom`` equal to the restatement's (fp32 and fp64) on seeded poses whose fp64
  crop edges lie more than 1e-2 px from an integer; ``bbox`` within 4 ulp of the restatement
  evaluated in fp32 in the contract's operation order (the kernel's own arithmetic; the distance to
  the fp64 evaluation is the projection's conditioning, printed, not bounded here); ``T`` and ``k``
  bit for bit the fp32 restatement's products.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import patch_restatement as pr

pytestmark = pytest.mark.gpu

S, H, W = 32, 48, 64
BOXES = [(10, 5, 29, 24),      # inside, upscale (crop 20)
         (8, 1, 52, 45),       # inside, downscale (crop 45)
         (30, 20, 45, 35),     # exact 2× (crop 16)
         (-7, -5, 13, 14),     # leaves the frame top-left; cw = ch + 1 = 21: nh = 30, top = 1
         (40, 25, 80, 64),     # leaves it bottom-right; cw = ch + 1 = 41: nh = 31
         (-10, -20, 79, 69),   # larger than the frame (crop 90)
         (0, 0, 0, 0),         # invalid
         (10, 5, 29, 24)]      # valid flag set, frame index outside the frames
FRAME_INDEX = [0, 1, 0, 1, 0, 1, 1, 7]
VALID = [1, 1, 1, 1, 1, 1, 0, 1]
MEAN, STD = [10.0, 20.0, 30.0], [58.395, 57.12, 57.375]
PAD = 128.0


def dev(a, dtype=None):
    x = torch.as_tensor(np.asarray(a))
    return (x if dtype is None else x.to(dtype)).cuda()


@lru_cache(maxsize=None)
def case():
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    geom = np.array([pr.geom_of(*b, S) if v else (0,) * 8 for b, v in zip(BOXES, VALID)], np.int32)
    assert tuple(geom[3, 4:]) == (32, 30, 0, 1) and tuple(geom[4, 4:]) == (32, 31, 0, 0)
    depth = rng.uniform(400.0, 2000.0, (2, H, W, 1)).astype(np.float32)
    mask = (rng.random((2, H, W, 1)) > 0.5).astype(np.uint8) * 255
    return dict(frames=frames, geom=geom, depth=depth, mask=mask,
                fidx=np.array(FRAME_INDEX, np.int32), valid=np.array(VALID, np.uint8))


@lru_cache(maxsize=None)
def gpu():
    c = case()
    return {k: dev(v) for k, v in c.items()}


@lru_cache(maxsize=None)
def restated(key="frames", dtype=np.float64, **kw):
    c = case()
    kw = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
    out = pr.extract_all(c[key], c["fidx"], c["geom"], c["valid"], S, dtype=dtype, **kw)
    out.setflags(write=False)
    return out


def run(key="frames", **kw):
    from scflow_amd import ops
    g = gpu()
    return ops.extract_patches(g[key], g["fidx"], g["geom"], g["valid"], S, **kw)


RGB = dict(pad=PAD, mean=tuple(MEAN), std=tuple(STD), to_rgb=True)


# ------------------------------------------------------------------------------ extract
def test_unquantised_bilinear_within_the_fp32_bound():
    got = run(quantize=False, **RGB).cpu().numpy().astype(np.float64)
    want = restated(quantize=False, **RGB)
    for c in range(3):
        err = np.abs(got[:, c] - want[:, c]).max()
        print(f"channel {c}: max |error| {err:.3e}, bound {2e-6 * 255 / STD[c]:.3e}")
        assert err <= 2e-6 * 255 / STD[c]


def test_exact_doubling_pad_pixels_and_invalid_patches_are_exact():
    got = run(quantize=False, **RGB).cpu().numpy()
    want32 = restated(dtype=np.float32, quantize=False, **RGB)
    assert np.array_equal(got[2], want32[2])  # 2×: weights 1/4, 3/4 on 8-bit levels
    pad = ((np.float32(PAD) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32))
    for i in (6, 7):  # invalid flag; frame index outside the frames
        assert np.array_equal(got[i], np.broadcast_to(pad[:, None, None], (3, S, S)))
    g = case()["geom"]
    for i in range(6):
        nw, nh, left, top = (int(v) for v in g[i, 4:])
        inner = np.zeros((S, S), bool)
        inner[top:top + nh, left:left + nw] = True
        for c in range(3):
            assert (got[i, c][~inner] == pad[c]).all()
            assert (got[i, c][inner] != pad[c]).any()
    same = sum(np.array_equal(got[i], want32[i]) for i in range(len(BOXES)))
    print(f"{same} of {len(BOXES)} patches equal the fp32 restatement bit for bit")


def test_channel_order():
    plain = dict(pad=PAD, quantize=True)
    bgr, rgb = run(to_rgb=False, **plain), run(to_rgb=True, **plain)
    assert torch.equal(rgb, bgr.flip(1))
    assert np.array_equal(bgr.cpu().numpy(), restated(dtype=np.float32, to_rgb=False, **plain))
    # mean / std are in output order
    m = run(to_rgb=True, pad=PAD, mean=MEAN, std=[1.0, 2.0, 4.0]).cpu()
    for c in range(3):
        assert torch.equal(m[:, c], (rgb[:, c].cpu() - MEAN[c]) / [1.0, 2.0, 4.0][c])


def test_quantised_levels():
    got = run(pad=PAD, quantize=True).cpu().numpy().astype(np.float64)
    exact = restated(pad=PAD, quantize=False)
    want = np.rint(exact)
    assert np.array_equal(got, np.rint(got)) and got.min() >= 0 and got.max() <= 255
    assert np.abs(got - want).max() <= 1
    clear = np.abs(exact - np.floor(exact) - 0.5) > 1e-3
    print(f"{(~clear).sum()} of {clear.size} pixels within 1e-3 of a half-integer; "
          f"{(got != want).sum()} differ from the fp64 rounding")
    assert np.array_equal(got[clear], want[clear])


def test_nearest_masks_are_exact():
    got = run("mask", pad=0.0, nearest=True).cpu().numpy()
    assert np.array_equal(got, restated("mask", dtype=np.float32, pad=0.0, nearest=True))
    assert set(np.unique(got)) == {0.0, 255.0}
    got3 = run(pad=PAD, nearest=True, to_rgb=True).cpu().numpy()
    assert np.array_equal(got3, restated(dtype=np.float32, pad=PAD, nearest=True, to_rgb=True))


def test_float_maps_bilinear():
    got = run("depth", pad=0.0, quantize=False).cpu().numpy().astype(np.float64)
    want = restated("depth", pad=0.0, quantize=False)
    bound = 2e-6 * float(case()["depth"].max())  # the image bound, scaled to the map's range
    err = np.abs(got - want).max()
    print(f"depth: max |error| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    u8 = run("mask", pad=0.0, quantize=False).cpu().numpy().astype(np.float64)
    assert np.abs(u8 - restated("mask", pad=0.0, quantize=False)).max() <= 2e-6 * 255


def test_extract_maps_wrapper():
    from scflow_amd import patches
    g = gpu()
    d = patches.extract_maps(g["depth"][..., 0], g["fidx"].long(), g["geom"], g["valid"] != 0, S)
    assert torch.equal(d, run("depth", pad=0.0, quantize=False))
    m = patches.extract_maps(g["mask"], g["fidx"], g["geom"], g["valid"], S, mode="nearest")
    assert torch.equal(m, run("mask", pad=0.0, nearest=True))


# ------------------------------------------------------------------------------ two routes
def _wide_case():
    """A 16×4096 frame and S = 32: a 4000-wide crop (12 003 bytes per row, beyond the 512 a band
    of 32 rows can stage) next to a 60-wide one (staged)."""
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (1, 16, 4096, 3), dtype=np.uint8)
    geom = np.array([(50, -92, 4049, 107) + pr.sizes(4000, 200, S), pr.geom_of(4030, -20, 4089, 39, S)],
                    np.int32)
    return frames, geom


def test_staged_and_direct_routes_give_the_same_bits(monkeypatch):
    from scflow_amd import _lib, ops
    frames, geom = _wide_case()

    def outputs():
        wide = ops.extract_patches(dev(frames), dev([0, 0], torch.int32), dev(geom),
                                   dev([1, 1], torch.uint8), S, quantize=False, **RGB)
        return [run(quantize=False, **RGB), run(pad=PAD), run("depth", pad=0.0, quantize=False),
                run("mask", pad=0.0, quantize=False), wide]

    assert not ops.patch_staged(20, 3, torch.uint8, S)  # the default: every tap read directly
    direct = outputs()
    monkeypatch.setenv("SCFLOW_PATCH_LDS", "1")
    _lib.reload_switches()
    try:
        for cw in (20, 45, 16, 21, 41, 90, 60):  # every crop of the cases but the wide one is staged
            assert ops.patch_staged(cw, 3, torch.uint8, S)
        assert ops.patch_staged(90, 1, torch.float32, S)
        assert not ops.patch_staged(4000, 3, torch.uint8, S)
        staged = outputs()
    finally:
        monkeypatch.delenv("SCFLOW_PATCH_LDS")
        _lib.reload_switches()
    for a, b in zip(direct, staged):
        assert torch.equal(a, b)


def test_crop_wider_than_the_budget():
    from scflow_amd import ops
    frames, geom = _wide_case()
    got = ops.extract_patches(dev(frames), dev([0, 0], torch.int32), dev(geom),
                              dev([1, 1], torch.uint8), S, quantize=False, **RGB)
    want = pr.extract_all(frames, [0, 0], geom, [1, 1], S, dtype=np.float64, quantize=False,
                          pad=PAD, mean=MEAN, std=STD, to_rgb=True)
    got = got.cpu().numpy().astype(np.float64)
    assert tuple(geom[0, 4:]) == (32, 2, 0, 15)
    for c in range(3):
        assert np.abs(got[:, c] - want[:, c]).max() <= 2e-6 * 255 / STD[c]


# ------------------------------------------------------------------------------ boxes
BH, BW = 480, 640


@lru_cache(maxsize=None)
def box_cases():
    """A 64-point table for 3 classes and seeded poses in front of a 480×640 camera; kept are the
    poses whose four fp64 crop edges lie more than 1e-2 px from an integer, so that truncation
    cannot differ between fp32 and fp64.  Objects near the left / top border give negative edges."""
    rng = np.random.default_rng(7)
    points = rng.uniform(-60.0, 60.0, (3, 64, 3)).astype(np.float32)
    counts = np.array([64, 40, 64], np.int32)
    Ks = np.array([[[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]],
                   [[1066.8, 0, 312.99], [0, 1067.5, 241.3], [0, 0, 1]]], np.float32)
    kept = []
    for _ in range(60):
        lab, fi = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        R = (q * np.sign(np.linalg.det(q))).astype(np.float32)
        tz = rng.uniform(500.0, 1500.0)
        t = np.array([rng.uniform(-0.6, 0.6) * tz, rng.uniform(-0.45, 0.45) * tz, tz], np.float32)
        ratio = np.float32(rng.uniform(1.0, 1.25))
        ref = pr.boxes(points[lab, :counts[lab]], R, t, Ks[fi], ratio, BH, BW, S, np.float64)
        if ref["edges"] is None:
            continue
        if min(abs(float(e) - round(float(e))) for e in ref["edges"]) <= 1e-2:
            continue
        kept.append(dict(label=lab, fi=fi, R=R, t=t, ratio=ratio, ref=ref))
    return points, counts, Ks, kept


def _run_boxes(kept, points, counts, Ks, k_per_frame=True):
    from scflow_amd import ops
    stack = lambda k, dt: dev(np.stack([c[k] for c in kept]), dt)  # noqa: E731
    fidx = dev([c["fi"] for c in kept], torch.int32)
    ori_k = dev(Ks) if k_per_frame else dev(Ks)[fidx.long()].contiguous()
    return ops.patch_boxes(dev(points), dev(counts), dev([c["label"] for c in kept], torch.int32),
                           stack("R", torch.float32), stack("t", torch.float32), ori_k,
                           stack("ratio", torch.float32), BH, BW, S, frame_index=fidx, num_frames=2,
                           k_per_frame=k_per_frame)


def test_boxes_match_the_restatement():
    points, counts, Ks, kept = box_cases()
    assert len(kept) >= 20
    assert any(c["ref"]["valid"] and min(c["ref"]["geom"][:2]) < 0 for c in kept)
    assert any(c["ref"]["valid"] and min(float(e) for e in c["ref"]["edges"]) < -1 for c in kept)
    bbox, geom, T, k, valid = (x.cpu().numpy() for x in _run_boxes(kept, points, counts, Ks))
    worst = 0.0
    for i, c in enumerate(kept):
        r64 = c["ref"]
        r32 = pr.boxes(points[c["label"], :counts[c["label"]]], c["R"], c["t"], Ks[c["fi"]],
                       c["ratio"], BH, BW, S, np.float32)
        assert bool(valid[i]) == r64["valid"] == r32["valid"], i
        assert tuple(geom[i]) == tuple(r64["geom"]) == tuple(r32["geom"]), i
        ulp = np.spacing(np.abs(r32["bbox"]).astype(np.float32))
        assert (np.abs(bbox[i].astype(np.float64) - r32["bbox"].astype(np.float64)) <= 4 * ulp).all(), i
        worst = max(worst, np.abs(bbox[i] - r64["bbox"]).max())
        # T and k from the same geometry and sf, bit for bit
        Tw, kw = pr.transform(geom[i], S, Ks[c["fi"]], np.float32) if valid[i] else \
            (np.eye(3, dtype=np.float32), Ks[c["fi"]])
        assert np.array_equal(T[i], Tw) and np.array_equal(k[i], kw), i
    print(f"{len(kept)} poses, {int(valid.sum())} valid; max |bbox - fp64 restatement| {worst:.3e} px")
    assert valid.sum() >= 10
    again = _run_boxes(kept, points, counts, Ks, k_per_frame=False)
    for a, b in zip((bbox, geom, T, k, valid), again):
        assert np.array_equal(a, b.cpu().numpy())


def test_boxes_invalid_objects():
    from scflow_amd import ops
    points, counts, Ks, _ = box_cases()
    I, K = np.eye(3, dtype=np.float32), Ks[0]
    rows = [  # label, frame, t, ratio → valid
        (0, 0, [0, 0, 900.0], 1.1, True),
        (0, 0, [0, 0, 30.0], 1.1, False),       # some points behind the camera (|X| ≤ 60)
        (0, 0, [0, 0, 1e7], 1.1, False),        # side·ratio < 1
        (0, 0, [0, 0, 61.0], 1.1, False),       # in front, but the crop exceeds 8192 px
        (0, 0, [3000.0, 0, 900.0], 1.1, False), # the crop misses the frame
        (0, 5, [0, 0, 900.0], 1.1, False),      # frame index outside [0, 2)
        (7, 0, [0, 0, 900.0], 1.1, False),      # label outside the table
        (0, 0, [0, 0, 900.0], float("nan"), False)]
    n = len(rows)
    Kn = np.repeat(K[None], n, 0)
    out = ops.patch_boxes(dev(points), dev(counts), dev([r[0] for r in rows], torch.int32),
                          dev(np.repeat(I[None], n, 0)), dev([r[2] for r in rows], torch.float32),
                          dev(Kn), dev([r[3] for r in rows], torch.float32), BH, BW, S,
                          frame_index=dev([r[1] for r in rows], torch.int32), num_frames=2)
    bbox, geom, T, k, valid = (x.cpu().numpy() for x in out)
    assert valid.tolist() == [int(r[4]) for r in rows]
    for i, r in enumerate(rows):
        if 0 <= r[0] < 3:
            ref = pr.boxes(points[r[0], :counts[r[0]]], I, np.asarray(r[2], np.float32), K, r[3],
                           BH, BW, S, np.float32, frame_ok=0 <= r[1] < 2)
            assert ref["valid"] == r[4] and tuple(geom[i]) == tuple(ref["geom"]), i
        if not r[4]:
            assert not geom[i].any() and np.array_equal(T[i], I) and np.array_equal(k[i], K), i


# ------------------------------------------------------------------------------ plumbing
def _pipeline():
    """Both ops back to back: boxes on the 480×640 cases, then patches of two synthetic frames."""
    from scflow_amd import ops
    points, counts, Ks, kept = box_cases()
    kept = kept[:8]
    frames = dev(np.random.default_rng(2).integers(0, 256, (2, BH, BW, 3), dtype=np.uint8))
    stack = lambda k, dt: dev(np.stack([c[k] for c in kept]), dt)  # noqa: E731
    args = (dev(points), dev(counts), dev([c["label"] for c in kept], torch.int32),
            stack("R", torch.float32), stack("t", torch.float32), dev(Ks),
            stack("ratio", torch.float32))
    fidx = dev([c["fi"] for c in kept], torch.int32)

    def go():
        bbox, geom, T, k, valid = ops.patch_boxes(*args, BH, BW, S, frame_index=fidx, num_frames=2,
                                                  k_per_frame=True)
        return bbox, geom, T, k, valid, ops.extract_patches(frames, fidx, geom, valid, S, **RGB)
    return go


def test_runs_on_the_current_stream():
    go = _pipeline()
    want = go()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = go()  # no synchronisation between the two launches
    s.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert want[4].any() and want[5].std() > 0


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
    with torch.cuda.graph(graph, stream=s):  # one chain: boxes → extract
        out = go()
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)


def test_no_objects():
    from scflow_amd import ops
    g = gpu()
    e = lambda *s, dt=torch.float32: torch.empty(*s, device="cuda", dtype=dt)  # noqa: E731
    points, counts, Ks, _ = box_cases()
    out = ops.patch_boxes(dev(points), dev(counts), e(0, dt=torch.int32), e(0, 3, 3), e(0, 3),
                          e(0, 3, 3), e(0), BH, BW, S)
    assert [tuple(o.shape) for o in out] == [(0, 4), (0, 8), (0, 3, 3), (0, 3, 3), (0,)]
    img = ops.extract_patches(g["frames"], e(0, dt=torch.int32), out[1], out[4], S)
    assert tuple(img.shape) == (0, 3, S, S)


def test_refusals_on_device_tensors():
    from scflow_amd import ops
    from scflow_amd._lib import ScflowError
    g = gpu()
    with pytest.raises(ScflowError, match="int32"):
        ops.extract_patches(g["frames"], g["fidx"].long(), g["geom"], g["valid"], S)
    with pytest.raises(ScflowError, match="contiguous"):
        ops.extract_patches(g["frames"].permute(0, 2, 1, 3), g["fidx"], g["geom"], g["valid"], S)
    with pytest.raises(ScflowError, match="entries"):
        ops.extract_patches(g["frames"], g["fidx"], g["geom"], g["valid"], S, mean=[0.0])
    with pytest.raises(ScflowError):
        ops.extract_patches(g["frames"].float(), g["fidx"], g["geom"], g["valid"], S)  # fp32 RGB


def test_opcheck_patch_ops():
    from scflow_amd import library  # noqa: F401  (registers the ops)
    g = gpu()
    points, counts, Ks, kept = box_cases()
    kept = kept[:4]
    stack = lambda k: dev(np.stack([c[k] for c in kept]), torch.float32)  # noqa: E731
    args = (dev(points), dev(counts), dev([c["label"] for c in kept]), stack("R"), stack("t"),
            dev(Ks), stack("ratio"), dev([c["fi"] for c in kept]), True, 2, BH, BW, S)
    torch.library.opcheck(torch.ops.scflow.patch_boxes.default, args)
    eargs = (g["frames"], g["fidx"], g["geom"], g["valid"], S, PAD, MEAN, STD, True, True, False)
    torch.library.opcheck(torch.ops.scflow.extract_patches.default, eargs)
    assert torch.equal(torch.ops.scflow.extract_patches(*eargs), run(**RGB))
