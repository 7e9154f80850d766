"""CPU: the training-patch contract's restatement (tests/train_patch_restatement.py) against
published known answers (Philox), scipy (normality, Euler order), ``colorsys`` (HSV) and hand
cases (blur); and the C ABI / ctypes / ops / torch.library layers of the new exports."""
import colorsys
import os
import re

import numpy as np
import pytest
import torch

from tests import train_patch_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("scflow_philox4x32", "scflow_train_draw", "scflow_train_patch_extract")

KNOWN = [  # counter, key → words, computed from the published algorithm
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]


# ------------------------------------------------------------------------------ generator
@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = tr.philox4x32(np.array(counter, np.uint64), np.array(key, np.uint64))
    assert [int(v) for v in got] == want
    from scflow_amd import ops
    assert list(ops.philox4x32(counter, key)) == want  # the library's own evaluation, on the host


def test_counter_layout():
    """(index, object, stream | step_hi << 8, step_lo) under (seed_lo, seed_hi)."""
    seed, step = 0x299f31d0a4093822, (0x13 << 32) | 0x03707344
    got = tr.words(0x243f6a88, 0x85a308d3, 7, seed, step)
    want = tr.philox4x32(np.array([0x243f6a88, 0x85a308d3, 7 | (0x13 << 8), 0x03707344], np.uint64),
                         np.array([0xa4093822, 0x299f31d0], np.uint64))
    assert np.array_equal(got, want)
    many = tr.words(np.arange(5), 3, tr.RNG_NOISE, 9, 1)
    assert many.shape == (5, 4) and np.array_equal(many[2], tr.words(2, 3, tr.RNG_NOISE, 9, 1))


def test_uniforms():
    w = np.array([0, 0xff, 0x100, 0xffffffff], np.uint32)
    assert tr.u01(w).tolist() == [0.0, 0.0, 2.0 ** -24, 1 - 2.0 ** -24]
    assert tr.u01_open(w, np.float64).tolist() == [2.0 ** -25, 2.0 ** -25, 1.5 * 2.0 ** -24,
                                                   1 - 2.0 ** -25]
    # fp32: 16777215.5 rounds to 2^24, so the largest word gives exactly 1 (a normal of 0)
    assert tr.u01_open(w).tolist() == [2.0 ** -25, 2.0 ** -25, 1.5 * 2.0 ** -24, 1.0]


def test_restated_normals_are_normal():
    stats = pytest.importorskip("scipy.stats")
    for dtype in (np.float32, np.float64):
        z = tr.normal3(tr.words(np.arange(20000), 5, tr.RNG_NOISE, 1234, 0), dtype)
        for j in range(3):
            p = stats.kstest(z[:, j].astype(np.float64), "norm").pvalue
            print(f"{dtype.__name__} normal {j}: KS p = {p:.3f}, mean {z[:, j].mean():+.4f}, "
                  f"std {z[:, j].std():.4f}")
            assert p > 1e-3
        c = np.corrcoef(z.T.astype(np.float64))
        assert np.abs(c - np.eye(3)).max() < 4 / np.sqrt(len(z))


def test_euler_order_is_scipys_zyx():
    Rot = pytest.importorskip("scipy.spatial.transform").Rotation
    rng = np.random.default_rng(0)
    for ang in rng.normal(0, 40, (20, 3)):
        want = Rot.from_euler("zyx", ang, degrees=True).as_matrix()
        assert np.abs(tr.euler_zyx(*ang) - want).max() < 1e-14
        assert np.abs(tr.euler_zyx(*ang[::-1]) - want).max() > 1e-3  # the opposite order is not


def test_draw_restatement_rejects_and_gives_up():
    X = np.random.default_rng(1).uniform(-60, 60, (40, 3))
    R, t = np.eye(3), np.array([0.0, 0.0, 900.0])
    d = tr.draw(X, 150.0, R, t, 0, 1, 0, tr.CFG)
    assert d["ok"] == 1 and d["tries"] >= 1 and d["rot"] <= 45 and d["trans"] <= 200 and d["add"] <= 1
    assert np.allclose(d["R"] @ d["R"].T, np.eye(3), atol=1e-12)
    tight = dict(tr.CFG, angle_limit=0.01)
    g = tr.draw(X, 150.0, R, t, 0, 1, 0, tight, max_tries=8)
    assert g["ok"] == 0 and g["tries"] == 8 and np.array_equal(g["R"], R) and g["add"] == 0
    off = dict(tr.CFG, angle_limit=-1, translation_limit=-1, add_limit=-1)
    assert tr.draw(X, 150.0, R, t, 0, 1, 0, off)["tries"] == 1
    ratio, row = tr.aug_row(0, 1, 0, tr.CFG)
    assert 1.0 <= ratio < 1.25 and 0.8 <= row[0] <= 1.2 and 0.5 <= row[1] <= 1.5
    assert 0 <= row[3] < 0.1 and row[4] in (1, 3, 5) and row[5] == 7 and not row[6:].any()
    assert tr.aug_row(0, 1, 0, dict(tr.CFG, p_hsv=-1, p_noise=-1, p_blur=-1))[1][5] == 0
    ks = {tr.aug_row(o, 1, 0, tr.CFG)[1][4] for o in range(40)}
    assert ks == {1, 3, 5}


# ------------------------------------------------------------------------------ stages
def test_integer_hsv_against_colorsys():
    rng = np.random.default_rng(2)
    px = rng.integers(0, 256, (5000, 3), dtype=np.uint8)
    px[:8] = [[0, 0, 0], [255, 255, 255], [7, 7, 7], [255, 0, 0], [0, 255, 0], [0, 0, 255],
              [10, 200, 200], [200, 10, 200]]
    h, s, v = tr.bgr_to_hsv(px)
    want = np.array([colorsys.rgb_to_hsv(r / 255, g / 255, b / 255) for b, g, r in px.tolist()])
    dh = np.abs(h - want[:, 0] * 180)
    dh = np.minimum(dh, 180 - dh)  # hue is circular
    ds = np.abs(s - want[:, 1] * 255)
    print(f"max |H - colorsys| {dh.max():.3f}, max |S - colorsys| {ds.max():.3f}")
    assert dh.max() <= 1 and ds.max() <= 1 and np.array_equal(v, px.max(1))
    assert h.min() >= 0 and h.max() <= 179 and s.max() <= 255


def test_hsv_round_trip_is_not_an_identity_but_stage_mask_zero_is():
    rng = np.random.default_rng(3)
    crop = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    for dtype in (np.float32, np.float64):
        back = tr.hsv_stage(crop, 1.0, 1.0, 1.0, dtype)
        d = np.abs(back.astype(int) - crop.astype(int))
        print(f"{dtype.__name__}: unit gains move a pixel by at most {d.max()} levels, "
              f"{d.mean():.3f} on average")
        assert 1 <= d.max() <= 5 and 0 < d.mean() <= 0.5  # 8-bit H (2° steps) loses information
    unit = np.array([1, 1, 1, 0, 1, tr.AUG_HSV, 0, 0], np.float32)
    assert not np.array_equal(tr.augment(crop, unit, 0, 1, 0), crop)
    none = np.array([0.5, 2.0, 0.1, 0.3, 5, 0, 0, 0], np.float32)
    assert tr.augment(crop, none, 0, 1, 0) is crop
    grey = np.full((2, 2, 3), 77, np.uint8)
    assert np.array_equal(tr.hsv_stage(grey, 1.1, 1.3, 1.0), grey)  # s = 0 stays grey
    # value gain 2 saturates: every channel of a grey pixel at 255
    assert (tr.hsv_stage(np.full((1, 1, 3), 200, np.uint8), 1.0, 1.0, 2.0) == 255).all()


def test_blur_by_hand():
    """A 3 × 4 crop, k = 5: rows fold −2, −1, 0, 1, 2, 3, 4 → 2, 1, 0, 1, 2, 1, 0 (period 4),
    columns −2 … 5 → 2, 1, 0, 1, 2, 3, 2, 1 (period 6)."""
    img = (np.arange(12, dtype=np.uint8).reshape(3, 4) * 7)[..., None].repeat(3, -1)
    assert tr.fold101(np.arange(-2, 5), 3).tolist() == [2, 1, 0, 1, 2, 1, 0]
    assert tr.fold101(np.arange(-2, 6), 4).tolist() == [2, 1, 0, 1, 2, 3, 2, 1]
    assert tr.fold101(np.arange(-2, 3), 1).tolist() == [0] * 5
    assert tr.fold101(np.arange(-2, 4), 2).tolist() == [0, 1, 0, 1, 0, 1]
    got = tr.blur_stage(img, 5)[..., 0]
    rows, cols = [2, 1, 0, 1, 2, 1, 0], [2, 1, 0, 1, 2, 3, 2, 1]
    for y in range(3):
        for x in range(4):
            total = sum(int(img[rows[y + dy], cols[x + dx], 0]) for dy in range(5) for dx in range(5))
            assert got[y, x] == (2 * total + 25) // 50  # round half up of total / 25
    assert got[0, 0] == (2 * (7 * sum(4 * r + c for r in [2, 1, 0, 1, 2] for c in [2, 1, 0, 1, 2]))
                         + 25) // 50
    assert tr.blur_stage(img, 1) is img
    flat = np.full((3, 4, 3), 9, np.uint8)
    assert np.array_equal(tr.blur_stage(flat, 3), flat)


def test_noise_restatement_clips_and_truncates():
    img = np.full((8, 8, 3), 128, np.uint8)
    vals = tr.noise_values(img, 0.1, 0, 1, 0, np.float64)
    out = tr.noise_stage(img, 0.1, 0, 1, 0, np.float64)
    assert np.array_equal(out, np.clip(vals, 0, 255).astype(np.uint8)) and out.std() > 10
    assert (tr.noise_stage(np.zeros_like(img), 0.5, 0, 1, 0) == 0).mean() > 0.3  # clipped below
    assert not np.array_equal(out, tr.noise_stage(img, 0.1, 1, 1, 0, np.float64))  # another object
    assert not np.array_equal(out, tr.noise_stage(img, 0.1, 0, 1, 1, np.float64))  # another step


# ------------------------------------------------------------------------------ plumbing
def test_header_signatures_and_library_agree_on_the_new_exports():
    from scflow_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scflow_hip.h")).read(),
                 flags=re.S)
    lib = _lib.load()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        args = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    define = lambda n: int(re.search(rf"#define\s+SCFLOW_{n}\s+(\d+)", src).group(1))  # noqa: E731
    assert define("TRAIN_CFG_LEN") == len(_lib.TRAIN_CFG) == 20
    for key, macro in (("angle_mean", "TRAIN_ANGLE_MEAN"), ("angle_std", "TRAIN_ANGLE_STD"),
                       ("x_mean", "TRAIN_T_MEAN"), ("x_std", "TRAIN_T_STD"),
                       ("angle_limit", "TRAIN_ANGLE_LIMIT"), ("translation_limit", "TRAIN_TRANS_LIMIT"),
                       ("add_limit", "TRAIN_ADD_LIMIT"), ("ratio_lo", "TRAIN_RATIO_LO"),
                       ("ratio_hi", "TRAIN_RATIO_HI"), ("h_ratio", "TRAIN_H_RATIO"),
                       ("noise_ratio", "TRAIN_NOISE_RATIO"), ("p_hsv", "TRAIN_P_HSV")):
        assert _lib.TRAIN_CFG.index(key) == define(macro), key
    assert (define("RNG_CROP"), define("RNG_COLOUR"), define("RNG_NOISE"), define("RNG_JITTER")) == \
        (_lib.RNG_CROP, _lib.RNG_COLOUR, _lib.RNG_NOISE, _lib.RNG_JITTER) == \
        (tr.RNG_CROP, tr.RNG_COLOUR, tr.RNG_NOISE, tr.RNG_JITTER)
    assert (define("AUG_HSV"), define("AUG_NOISE"), define("AUG_BLUR")) == \
        (_lib.AUG_HSV, _lib.AUG_NOISE, _lib.AUG_BLUR) == (tr.AUG_HSV, tr.AUG_NOISE, tr.AUG_BLUR)
    assert define("PATCH_AUG_DIRECT") == _lib.PATCH_AUG_DIRECT
    assert define("TRAIN_MAX_TRIES") == _lib.TRAIN_MAX_TRIES
    from scflow_amd import patches
    assert patches.TRAIN_AUG == tr.CFG


def test_argument_errors_are_codes_before_any_launch():
    from scflow_amd import _lib
    lib = _lib.load()
    one = 1  # any non-null address: the checks come before anything is dereferenced
    draw = lambda ptrs, *ints: lib.scflow_train_draw(*ptrs, *ints, None)  # noqa: E731
    assert draw([None] * 14, 1, 1, 8, 32, 5, 0, 0, 0) == -1
    assert draw([one] * 14, 0, 1, 8, 32, 5, 0, 0, 0) == -1           # n = 0
    assert draw([one] * 14, 1, 1, 8, 32, 7, 0, 0, 0) == -2           # kernel side above 5
    assert draw([one] * 14, 1, 1, 8, 225, 5, 0, 0, 0) == -2          # more tries than streams
    assert draw([one] * 14, 1, 1, 8, 32, 5, 0, 1 << 56, 0) == -2     # step beyond 56 bits
    ext = lambda ptrs, *rest: lib.scflow_train_patch_extract(*ptrs, *rest, None)  # noqa: E731
    assert ext([None] * 6, 1, 1, 48, 64, 32, 128, None, None, 0, 0, 0, 0) == -1
    assert ext([one] * 6, 1, 1, 48, 64, 32, 256, None, None, 0, 0, 0, 0) == -1   # pad not a level
    assert ext([one] * 6, 1, 1, 48, 64, 32, 128, None, None, 4, 0, 0, 0) == -1   # NEAREST: no
    assert ext([one] * 6, 1, 1, 48, 64, 30, 128, None, None, 0, 0, 0, 0) == -2   # side % 4
    assert ext([16] * 5 + [8], 1, 1, 48, 64, 32, 128, None, None, 0, 0, 0, 0) == -3  # alignment


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


@pytest.mark.parametrize("n", [5, 0])
def test_fake_implementations_give_shapes_and_dtypes(n):
    from scflow_amd import library  # noqa: F401  (registers the ops)
    from scflow_amd._lib import TRAIN_CFG
    i32, f32 = torch.int32, torch.float32
    cfg = [float(tr.CFG[k]) for k in TRAIN_CFG]
    out = torch.ops.scflow.train_draw(_meta(3, 64, 3), _meta(3, dtype=i32), _meta(n, dtype=torch.long),
                                      _meta(3), _meta(n, 3, 3), _meta(n, 3), cfg, 5, 32, 1, 0, 0)
    assert [(tuple(o.shape), o.dtype) for o in out] == [
        ((n, 3, 3), f32), ((n, 3), f32), ((n, 3), f32), ((n,), torch.uint8), ((n,), i32),
        ((n,), f32), ((n, 8), f32)]
    img = torch.ops.scflow.patch_extract_aug(_meta(2, 48, 64, 3, dtype=torch.uint8),
                                             _meta(n, dtype=i32), _meta(n, 8, dtype=i32),
                                             _meta(n, dtype=torch.uint8), out[6], 32, 1, 0, 0, 128,
                                             None, None, True, True)
    assert tuple(img.shape) == (n, 3, 32, 32) and img.dtype == f32


def test_ops_refuse_before_device_work():
    from scflow_amd import ops, patches
    from scflow_amd._lib import ScflowError
    i32 = torch.int32
    pts, cnt, lab = torch.zeros(3, 64, 3), torch.full((3,), 64, dtype=i32), torch.zeros(2, dtype=i32)
    R, t, diam = torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3), torch.ones(3)
    with pytest.raises(ScflowError, match="is on cpu"):
        ops.train_draw(pts, cnt, lab, diam, R, t, tr.CFG, 1, 0)
    frames = torch.zeros(2, 48, 64, 3, dtype=torch.uint8)
    geom, valid, aug = torch.zeros(2, 8, dtype=i32), torch.ones(2, dtype=torch.uint8), torch.zeros(2, 8)
    with pytest.raises(ScflowError, match="is on cpu"):
        ops.extract_patches_aug(frames, lab, geom, valid, aug, 32, 1, 0)
    with pytest.raises(ScflowError, match="multiple of 4"):
        ops.extract_patches_aug(frames, lab, geom, valid, aug, 30, 1, 0)
    with pytest.raises(ScflowError, match="is on cpu"):
        patches.frames_to_train_patches(frames, frames[..., 0], lab, R, t, R, lab, pts, cnt, diam,
                                        1, 0, size=32)
    with pytest.raises(ScflowError, match="step"):
        ops._require_counter(1, 1 << 56, 0)
    with pytest.raises(ScflowError, match="object_offset"):
        ops._require_counter(1, 0, 1 << 32)
    with pytest.raises(ScflowError, match="seed"):
        ops._require_counter(-1, 0, 0)
    ops._require_counter(2 ** 64 - 1, 2 ** 56 - 1, 2 ** 32 - 1)
