"""CPU: the patch contract's restatement (tests/patch_restatement.py) against a hand-worked case,
Pillow's bilinear resize and its own integer size formula; T's inverse; and the C ABI / ctypes /
ops / torch.library layers of the new exports (symbols, fake implementations, refusals before
device work, N = 0)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import patch_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH_EXPORTS = ("scflow_patch_boxes", "scflow_patch_extract", "scflow_patch_staged")


# ------------------------------------------------------------------------------ hand case
def test_hand_worked_case_leaving_the_top_left_corner():
    """A 6×8 frame with value 10·y + x, S = 8.  Two model points at z = 1 under K = I project to
    (−1.5, −1) and (2.5, 2): side = max(4, 3) = 4, centre (0.5, 0.5), ratio 1 → half = 2, edges
    −1.5 and 2.5 on both axes, truncated TOWARD ZERO to −1 and 2 (a floor would give −2): a 4×4
    crop one pixel outside the frame at the top and the left, m = 4, sf = 2, nw = nh = 8, no
    padding.  Output x samples the crop at (2·dx − 1)/4 = −0.25 (clamped to 0), 0.25, 0.75, …,
    2.75, 3.25 (clamped to 3): the rows of W below."""
    H, W_, S, pad = 6, 8, 8, 100.0
    frame = (10 * np.arange(H)[:, None] + np.arange(W_)[None, :]).astype(np.uint8)[..., None]
    pts = np.array([[-1.5, -1.0, 1.0], [2.5, 2.0, 1.0]])
    for dtype in (np.float32, np.float64):
        bx = pr.boxes(pts, np.eye(3), np.zeros(3), np.eye(3), 1.0, H, W_, S, dtype)
        assert bx["valid"] and bx["bbox"].tolist() == [-1.5, -1.0, 2.5, 2.0]
        assert [float(e) for e in bx["edges"]] == [-1.5, -1.5, 2.5, 2.5]
        assert bx["geom"] == (-1, -1, 2, 2, 8, 8, 0, 0)
        assert bx["T"].tolist() == [[2, 0, 2], [0, 2, 2], [0, 0, 1]]
        assert bx["k"].tolist() == bx["T"].tolist()  # K = I
        crop = pr.crop(frame, -1, -1, 2, 2, pad, dtype)[..., 0]
        assert crop.tolist() == [[100, 100, 100, 100], [100, 0, 1, 2], [100, 10, 11, 12],
                                 [100, 20, 21, 22]]
        Wm = np.array([[1, 0, 0, 0], [.75, .25, 0, 0], [.25, .75, 0, 0], [0, .75, .25, 0],
                       [0, .25, .75, 0], [0, 0, .75, .25], [0, 0, .25, .75], [0, 0, 0, 1]])
        want = Wm @ crop.astype(np.float64) @ Wm.T  # dyadic weights on small integers: exact
        got = pr.extract(frame, bx["geom"], True, S, pad=pad, quantize=False, dtype=dtype)[0]
        assert got.dtype == dtype and np.array_equal(got, want)
        assert got[0, 0] == 100 and got[7, 7] == 22 and got[1, 1] == 93.75 and got[3, 3] == 2.75
        q = pr.extract(frame, bx["geom"], True, S, pad=pad, quantize=True, dtype=dtype)[0]
        assert np.array_equal(q, np.rint(want)) and q[1, 1] == 94 and q[3, 3] == 3
        # normalisation and an invalid object
        n = pr.extract(frame, bx["geom"], True, S, pad=pad, mean=[4.0], std=[2.0], quantize=False,
                       dtype=dtype)[0]
        assert np.array_equal(n, (want - 4) / 2)
        assert (pr.extract(frame, bx["geom"], False, S, pad=pad, mean=[4.0], std=[2.0],
                           dtype=dtype) == 48).all()


def test_padding_and_channel_order():
    """A 3×5 crop (cw = 5, ch = 3) in S = 8: m = 5, nw = 8, nh = int(3·1.6 + 0.5) = 5, left = 0,
    top = 1; rows 0 and 6, 7 are padding.  to_rgb reverses the channels before mean / std."""
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    g = pr.geom_of(2, 1, 6, 3, 8)
    assert g == (2, 1, 6, 3, 8, 5, 0, 1)
    mean, std = [1.0, 2.0, 3.0], [2.0, 4.0, 8.0]
    a = pr.extract(frame, g, True, 8, pad=7.0, mean=mean, std=std, to_rgb=True)
    b = pr.extract(frame, g, True, 8, pad=7.0, to_rgb=False)
    for c in range(3):
        assert np.array_equal(a[c], (b[2 - c] - np.float32(mean[c])) / np.float32(std[c]))
        assert (b[c, 0] == 7).all() and (b[c, 6:] == 7).all() and not (b[c, 1:6] == 7).all()
    # the nearest route keeps source values
    m = pr.extract(frame[..., :1], g, True, 8, pad=0.0, nearest=True)[0]
    assert set(np.unique(m[1:6])) <= set(np.unique(frame[1:4, 2:7, 0]).astype(np.float32))
    assert m[1, 0] == frame[1, 2, 0] and m[5, 7] == frame[3, 6, 0]


# ------------------------------------------------------------------------------ Pillow
@pytest.mark.parametrize("src,dst", [((20, 20), (32, 32)), ((23, 24), (31, 32)),
                                     ((21, 20), (32, 30)), ((13, 29), (14, 32))])
def test_upscales_within_one_level_of_pillow(src, dst):
    """(h, w) → (nh, nw).  Pillow resamples in two passes and rounds to uint8 between them, so
    equality is not expected: at most one level anywhere."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(src[0] * 100 + src[1])
    img = rng.integers(0, 256, src + (3,), dtype=np.uint8)
    want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BILINEAR), np.float64)
    for dtype in (np.float32, np.float64):
        got = np.rint(pr.resize_linear(img, dst[1], dst[0], dtype))
        diff = np.abs(got - want).max()
        print(f"{src} -> {dst} {dtype.__name__}: max |restatement - Pillow| = {diff} levels")
        assert diff <= 1.0


# ------------------------------------------------------------------------------ size formula
def test_integer_sizes_equal_the_float_formula():
    """nw = (2·cw·S + m) div 2m is mmcv's int(cw · (S / m) + 0.5) in Python floats wherever the
    two crop sides differ by at most one (what max(r−l, b−t) on both axes produces)."""
    for S in (32, 256):
        for cw in range(1, 601):
            for ch in range(max(1, cw - 1), min(600, cw + 1) + 1):
                m = max(cw, ch)
                sf = S / m
                nw, nh, left, top = pr.sizes(cw, ch, S)
                assert (nw, nh) == (int(cw * sf + 0.5), int(ch * sf + 0.5)), (cw, ch, S)
                assert 1 <= nw <= S and 1 <= nh <= S and max(nw, nh) == S
                assert (left, top) == ((S - nw) // 2, (S - nh) // 2)


# ------------------------------------------------------------------------------ T
@pytest.mark.parametrize("box", [(10, 5, 29, 24), (-7, -5, 13, 14), (40, 25, 80, 64),
                                 (-10, -20, 79, 69)])
def test_inverse_of_t_maps_the_patch_back_to_the_crop_box(box):
    S = 32
    g = pr.geom_of(*box, S)
    x1, y1, x2, y2, nw, nh, left, top = g
    K = np.array([[600.0, 0, 31.5], [0, 598.0, 23.25], [0, 0, 1]])
    T, k = pr.transform(g, S, K, np.float32)
    Ti = np.linalg.inv(T.astype(np.float64))
    sf = S / max(x2 - x1 + 1, y2 - y1 + 1)
    corners = np.array([[left, top, 1.0], [left + sf * (x2 - x1 + 1), top + sf * (y2 - y1 + 1), 1.0]])
    back = corners @ Ti.T
    # fp32 T: sf and the two offsets carry one rounding each, on coordinates below 100 px
    np.testing.assert_allclose(back[:, :2], [[x1, y1], [x2 + 1, y2 + 1]], atol=1e-4)
    # k projects a camera point where T sends its projection under K
    X = np.array([12.0, -7.0, 640.0])
    p, q = K @ X, k.astype(np.float64) @ X
    np.testing.assert_allclose(q[:2] / q[2], (T.astype(np.float64) @ (p / p[2]))[:2], atol=1e-4)


# ------------------------------------------------------------------------------ PyTorch loop
def test_torch_loop_agrees_with_the_restatement():
    """The benchmark's per-object PyTorch version computes the same patches (its source
    coordinates are floats, not exact rationals: compared before quantisation)."""
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    boxes = [(10, 5, 29, 24), (8, 1, 52, 45), (-7, -5, 13, 14), (40, 25, 80, 64)]
    geom = np.array([pr.geom_of(*b, 32) for b in boxes] + [[0] * 8])
    fidx, valid = np.array([0, 1, 1, 0, 0]), np.array([1, 1, 1, 1, 0])
    kw = dict(pad=128.0, mean=[1.0, 2.0, 3.0], std=[50.0, 60.0, 70.0], to_rgb=True, quantize=False)
    want = pr.extract_all(frames, fidx, geom, valid, 32, dtype=np.float64, **kw)
    got = pr.torch_patches(torch.from_numpy(frames), torch.from_numpy(fidx), torch.from_numpy(geom),
                           torch.from_numpy(valid), 32, **kw).numpy()
    assert np.abs(got - want).max() <= 1e-3 / 50


# ------------------------------------------------------------------------------ plumbing
def test_header_signatures_and_library_agree_on_the_patch_exports():
    from scflow_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scflow_hip.h")).read(),
                 flags=re.S)
    assert set(re.findall(r"\b(scflow_patch_[a-z0-9_]+)\s*\(", src)) == set(PATCH_EXPORTS)
    assert re.search(r"#define\s+SCFLOW_ABI_VERSION\s+4\b", src)
    m = re.search(r"#define\s+SCFLOW_PATCH_MAX_CROP\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.PATCH_MAX_CROP == pr.MAX_CROP
    for name, val in (("U8", _lib.PATCH_U8), ("F32", _lib.PATCH_F32), ("TO_RGB", _lib.PATCH_TO_RGB),
                      ("QUANTIZE", _lib.PATCH_QUANTIZE), ("NEAREST", _lib.PATCH_NEAREST)):
        assert int(re.search(rf"#define\s+SCFLOW_PATCH_{name}\s+(\d+)", src).group(1)) == val
    lib = _lib.load()
    assert lib.scflow_abi_version() == 4 == _lib.ABI_VERSION
    for name in PATCH_EXPORTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        args = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_argument_errors_are_codes_before_any_launch():
    from scflow_amd import _lib
    lib = _lib.load()
    assert lib.scflow_patch_boxes(*([None] * 13), 1, 1, 8, 0, 1, 48, 64, 32, None) == -1
    assert lib.scflow_patch_extract(*([None] * 5), 1, 1, 48, 64, 3, 0, 32, 128.0, None, None, 0,
                                    None) == -1
    one = 1  # any non-null address: the shape checks come before anything is dereferenced
    assert lib.scflow_patch_boxes(*([one] * 13), 1, 1, 8, 0, 1, 48, 64, 30, None) == -2  # side % 4
    assert lib.scflow_patch_boxes(*([one] * 13), 0, 1, 8, 0, 1, 48, 64, 32, None) == -1  # n = 0
    assert lib.scflow_patch_boxes(*([one] * 6), None, *([one] * 6), 1, 1, 8, 1, 1, 48, 64, 32,
                                  None) == -1  # K per frame without frame_index
    assert lib.scflow_patch_extract(*([one] * 5), 1, 1, 48, 64, 2, 0, 32, 0.0, None, None, 0,
                                    None) == -2  # two channels
    assert lib.scflow_patch_extract(*([one] * 5), 1, 1, 48, 64, 3, 1, 32, 0.0, None, None, 0,
                                    None) == -2  # float32 frames are single-channel
    assert lib.scflow_patch_extract(*([one] * 5), 1, 1, 48, 64, 3, 0, 32, 0.0, None, None, 8,
                                    None) == -1  # unknown flag
    assert lib.scflow_patch_extract(*([16] * 4), 8, 1, 1, 48, 64, 3, 0, 32, 0.0, None, None, 0,
                                    None) == -3  # out not 16-byte aligned


def test_staging_query_follows_the_budget_and_the_switch(monkeypatch):
    """32 KiB for two source rows per output row of a band: at S = 32 a band is the whole patch
    (32 rows), so a row of pad16(3·cw + 3) bytes is staged up to 512 bytes; at S = 256 (4 rows) up
    to 4096 bytes."""
    from scflow_amd import _lib, ops
    _lib.reload_switches()
    assert not ops.patch_staged(20, 3, torch.uint8, 32)  # the default reads every crop directly
    with pytest.raises(_lib.ScflowError):
        ops.patch_staged(20, 2, torch.uint8, 32)
    monkeypatch.setenv("SCFLOW_PATCH_LDS", "1")
    try:
        assert not ops.patch_staged(20, 3, torch.uint8, 32)  # cached until the reload
        _lib.reload_switches()
        assert ops.patch_staged(20, 3, torch.uint8, 32) and ops.patch_staged(90, 3, torch.uint8, 32)
        assert ops.patch_staged(169, 3, torch.uint8, 32) and not ops.patch_staged(170, 3, torch.uint8, 32)
        assert ops.patch_staged(1364, 3, torch.uint8, 256) and not ops.patch_staged(1365, 3, torch.uint8, 256)
        assert ops.patch_staged(1023, 1, torch.float32, 256)
        assert not ops.patch_staged(1024, 1, torch.float32, 256)
        assert not ops.patch_staged(4000, 3, torch.uint8, 32)
    finally:
        monkeypatch.delenv("SCFLOW_PATCH_LDS")
        _lib.reload_switches()
    assert not ops.patch_staged(20, 3, torch.uint8, 32)


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


@pytest.mark.parametrize("n", [5, 0])
def test_fake_implementations_give_shapes_and_dtypes(n):
    from scflow_amd import library  # noqa: F401  (registers the ops)
    i32 = torch.int32
    out = torch.ops.scflow.patch_boxes(_meta(3, 64, 3), _meta(3, dtype=i32), _meta(n, dtype=torch.long),
                                       _meta(n, 3, 3), _meta(n, 3), _meta(2, 3, 3), _meta(n),
                                       _meta(n, dtype=torch.long), True, 2, 48, 64, 32)
    assert [(tuple(o.shape), o.dtype) for o in out] == [
        ((n, 4), torch.float32), ((n, 8), i32), ((n, 3, 3), torch.float32),
        ((n, 3, 3), torch.float32), ((n,), torch.uint8)]
    for frames, c in ((_meta(2, 48, 64, 3, dtype=torch.uint8), 3), (_meta(2, 48, 64, 1), 1)):
        img = torch.ops.scflow.extract_patches(frames, _meta(n, dtype=i32), out[1], out[4], 32,
                                               128.0, None, None, c == 3, True, False)
        assert tuple(img.shape) == (n, c, 32, 32) and img.dtype == torch.float32


def test_ops_refuse_before_device_work():
    """CPU tensors, wrong dtypes, strides and shapes all raise ScflowError: on this path no
    launch is reached (there is no device in this test)."""
    from scflow_amd import ops, patches
    from scflow_amd._lib import ScflowError
    i32 = torch.int32
    pts, cnt, lab = torch.zeros(3, 64, 3), torch.full((3,), 64, dtype=i32), torch.zeros(2, dtype=i32)
    R, t, K, ratio = torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3), torch.eye(3).repeat(2, 1, 1), \
        torch.ones(2)
    with pytest.raises(ScflowError, match="is on cpu"):
        ops.patch_boxes(pts, cnt, lab, R, t, K, ratio, 48, 64, 32)
    with pytest.raises(ScflowError, match="multiple of 4"):
        ops.patch_boxes(pts, cnt, lab, R, t, K, ratio, 48, 64, 30)
    frames = torch.zeros(2, 48, 64, 3, dtype=torch.uint8)
    geom, valid = torch.zeros(2, 8, dtype=i32), torch.ones(2, dtype=torch.uint8)
    with pytest.raises(ScflowError, match="is on cpu"):
        ops.extract_patches(frames, lab, geom, valid, 32)
    with pytest.raises(ScflowError, match="is on cpu"):
        patches.frames_to_patches(frames, lab, R, t, K, lab, pts, cnt, size=32)
    with pytest.raises(ScflowError, match="mode"):
        patches.extract_maps(frames[..., 0], lab, geom, mode="cubic")
    # the dtype / contiguity / shape refusals come from one checker; drive it directly, with a
    # stand-in for the device test so the later branches are reached without a GPU
    class OnDevice(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)
    dev = lambda x: x.as_subclass(OnDevice)  # noqa: E731
    ops._require_patch(dev(geom), "geom", i32, (2, 8))
    with pytest.raises(ScflowError, match="must be torch.int32"):
        ops._require_patch(dev(geom.long()), "geom", i32, (2, 8))
    with pytest.raises(ScflowError, match="contiguous"):
        ops._require_patch(dev(frames.permute(0, 3, 1, 2)), "frames", torch.uint8)
    with pytest.raises(ScflowError, match=r"\[2, 8\]"):
        ops._require_patch(dev(geom[:, :4].contiguous()), "geom", i32, (2, 8))
    with pytest.raises(ScflowError, match="tensor"):
        ops._require_patch(None, "frames", torch.uint8)


def test_point_table_takes_every_vertex():
    from scflow_amd import patches, synthetic
    from scflow_amd.renderer import Renderer
    meshes = {1: synthetic.ellipsoid_mesh((30.0, 20.0, 10.0), 6, 8),
              3: synthetic.ellipsoid_mesh((30.0, 20.0, 10.0), 4, 6)}
    r = Renderer(image_size=(32, 32), soft_blending=False, render_mask=False, meshes=meshes)
    points, counts = patches.point_table(r)
    n1, n3 = len(meshes[1][0]), len(meshes[3][0])
    assert tuple(points.shape) == (4, max(n1, n3), 3) and points.dtype == torch.float32
    assert counts.dtype == torch.int32 and counts.tolist() == [0, n1, 0, n3]
    assert np.array_equal(points[3, :n3].numpy(), np.asarray(meshes[3][0], np.float32))
    assert not points[3, n3:].any() and not points[0].any()
