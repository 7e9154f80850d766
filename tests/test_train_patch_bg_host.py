"""CPU: the background stage's restatement (tests/train_patch_bg_restatement.py)
against hand-evaluated draws, its own statistics and hand cases of the sample and the select; and
the C ABI / ctypes / ops / torch.library / patches layers of scflow_train_patch_extract_bg."""
import os
import re

import numpy as np
import pytest
import torch

from tests import patch_restatement as pr
from tests import train_patch_bg_restatement as bg
from tests import train_patch_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "scflow_train_patch_extract_bg"

# (seed, step, object) → words 0 and 1 of counter (0, object, 3 | step_hi << 8, step_lo), and by
# hand from them: u = (w >> 8)·2^-24; taken at p = 0.3 where u0 ≤ 0.3; slot = int(u1·7)
DRAWS = [
    # u0 = 0x3fb17e / 2^24 = 0.24880 ≤ 0.3; u1 = 0x5d2c92 / 2^24 = 0.36396, ·7 = 2.548 → 2
    ((0x299f31d0a4093822, (0x13 << 32) | 0x03707344, 0x85a308d3), (0x3fb17ef2, 0x5d2c92e8), 2, 2),
    # u0 = 0x05fd91 / 2^24 = 0.02340 ≤ 0.3; u1 = 0xf89e4c / 2^24 = 0.97117, ·7 = 6.798 → 6
    ((99, 4, 1), (0x05fd9130, 0xf89e4c77), 6, 6),
    # u0 = 0xc42712 / 2^24 = 0.76622 > 0.3: none; at p = 1: u1 = 0x2df328 / 2^24 = 0.17949, ·7 = 1.256 → 1
    ((77, 2, 5), (0xc427120c, 0x2df32898), -1, 1)]


# ------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("triple,w01,at_03,at_1", DRAWS)
def test_draw_against_hand_evaluated_words(triple, w01, at_03, at_1):
    seed, step, obj = triple
    w = tr.words(0, obj, bg.RNG_BACKGROUND, seed, step)
    assert (int(w[0]), int(w[1])) == w01
    from scflow_amd import ops  # the library's own evaluation of the same counter, on the host
    lib = ops.philox4x32([0, obj, 3 | ((step >> 32) << 8), step & 0xFFFFFFFF],
                         [seed & 0xFFFFFFFF, seed >> 32])
    assert tuple(lib[:2]) == w01
    for dtype in (np.float32, np.float64):
        assert bg.draw(obj, seed, step, 0.3, 7, dtype) == at_03
        assert bg.draw(obj, seed, step, 1.0, 7, dtype) == at_1
        assert bg.draw(obj, seed, step, 1.0, 1, dtype) == 0
    # another stream, another answer: the colour draws do not move with it
    assert not np.array_equal(w, tr.words(0, obj, tr.RNG_COLOUR, seed, step))


def test_draw_statistics_over_4096_objects():
    n, p, slots = 4096, 0.3, 7
    s = np.array([bg.draw(o, 12345, 3, p, slots) for o in range(n)])
    k = int((s >= 0).sum())
    sigma = np.sqrt(n * p * (1 - p))
    print(f"{k} of {n} replaced (mean {n * p:.1f}, 4 sigma {4 * sigma:.1f})")
    assert abs(k - n * p) <= 4 * sigma
    hits = np.bincount(s[s >= 0], minlength=slots)
    sig = np.sqrt(k * (1 / slots) * (1 - 1 / slots))
    print(f"slots {hits.tolist()} (mean {k / slots:.1f}, 4 sigma {4 * sig:.1f})")
    assert len(hits) == slots and (np.abs(hits - k / slots) <= 4 * sig).all()
    assert all(bg.draw(o, 12345, 3, 1.0, slots) >= 0 for o in range(64))
    # u = 0 has probability 2^-24: p = 0 takes nothing here
    assert all(bg.draw(o, 12345, 3, 0.0, slots) == -1 for o in range(n))


def test_override_entries():
    sizes = np.array([[24, 40], [17, 33], [25, 2], [0, 5]], np.int32)
    assert [bg.chosen(v, 4) for v in (-1, 0, 3, 4, -2, 99)] == [-1, 0, 3, -1, -1, -1]
    assert [bg.chosen(v, 4, sizes, (24, 40)) for v in range(4)] == [0, 1, -1, -1]


# ------------------------------------------------------------------------------ sample and select
def test_background_sample_by_hand():
    """A 2 × 3 image to a 4 × 6 crop is an exact 2×: weights 1/4, 3/4 (exact in fp32), the edges
    clamp; to its own size it is itself; one used pixel fills the crop."""
    img = np.array([[[0, 10, 20], [40, 50, 60], [200, 210, 220]],
                    [[80, 90, 100], [120, 130, 140], [240, 250, 255]]], np.uint8)
    for dtype in (np.float32, np.float64):
        assert np.array_equal(bg.background_crop(img, 3, 2, dtype), img)
        up = bg.background_crop(img, 6, 4, dtype)
        assert up.shape == (4, 6, 3)
        assert np.array_equal(up[0, 0], img[0, 0]) and np.array_equal(up[3, 5], img[1, 2])
        # output (1, 1): y = 0.25, x = 0.25 →
        # 0.75·(0.75·0 + 0.25·40) + 0.25·(0.75·80 + 0.25·120) = 7.5 + 22.5
        assert up[1, 1, 0] == 30
        # output column 2 of row 0: x = 0.75 → 0.25·0 + 0.75·40 = 30
        assert up[0, 2, 0] == 30
        one = bg.background_crop(img[:1, :1], 5, 7, dtype)
        assert one.shape == (7, 5, 3) and (one == img[0, 0]).all()
    pool = np.zeros((2, 4, 5, 3), np.uint8)
    pool[1, :2, :3] = img
    assert np.array_equal(bg.used(pool, np.array([[4, 5], [2, 3]]), 1), img)
    assert bg.used(pool, None, 1).shape == (4, 5, 3)


def test_fp32_and_fp64_samples_differ_by_at_most_one_level_on_half_a_percent():
    """The bound the GPU test puts on the kernel against the fp64 restatement, between the two
    restatements alone, on that test's pool, used sizes and crops."""
    from tests import train_patch_bg_cases as cs
    c = cs.case()
    for slot in range(cs.SLOTS):
        image = bg.used(c["pool"], c["sizes"], slot)
        assert image.shape[:2] == cs.SIZES[slot]
        diff = total = 0
        for i in cs.LIVE:
            x1, y1, x2, y2 = cs.BOXES[i]
            a = bg.background_crop(image, x2 - x1 + 1, y2 - y1 + 1, np.float32).astype(int)
            b = bg.background_crop(image, x2 - x1 + 1, y2 - y1 + 1, np.float64).astype(int)
            assert np.abs(a - b).max() <= 1
            diff, total = diff + int((a != b).sum()), total + a.size
        print(f"slot {slot}: {diff} of {total} background levels differ between the fp32 and fp64 "
              f"samples ({diff / total:.3%})")
        assert diff / total <= 0.005
    # and after the resize to S = 32, which is what the GPU test compares
    rows = np.zeros((len(cs.BOXES), 8), np.float32)
    for slot in range(cs.SLOTS):
        image = bg.used(c["pool"], c["sizes"], slot)
        out = [[bg.extract_aug_bg(c["frames"][0], c["zeros"][0], cs.geoms()[i], rows[i], i, cs.S, 1, 0,
                                  image, d) for i in cs.LIVE] for d in (np.float32, np.float64)]
        d = np.abs(np.array(out[0], np.float64) - np.array(out[1]))
        print(f"slot {slot}: {(d > 0).mean():.3%} of the patch levels differ, by up to {d.max():.0f}")
        assert d.max() <= 1 and (d > 0).mean() <= 0.005


def test_select_by_hand():
    frame = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3)
    mask = np.zeros((4, 5), np.uint8)
    mask[1, 2], mask[3, 4] = 255, 1  # any nonzero byte is foreground
    fg = bg.foreground(mask, -1, 0, 5, 4)  # a 7 × 5 crop leaving the frame left, right and below
    assert fg.shape == (5, 7) and fg.sum() == 2 and fg[1, 3] and fg[3, 5]
    image = np.full((3, 3, 3), 9, np.uint8)
    geom = pr.geom_of(-1, 0, 5, 4, 8)
    out = bg.composite_crop(frame, mask, geom, image, pad=128)
    assert np.array_equal(out[1, 3], frame[1, 2]) and np.array_equal(out[3, 5], frame[3, 4])
    out[1, 3], out[3, 5] = 9, 9
    assert (out == 9).all()  # pad pixels and masked-out frame pixels alike
    plain = bg.composite_crop(frame, mask, geom, None, pad=128)
    assert np.array_equal(plain, pr.crop(frame, -1, 0, 5, 4, 128, np.uint8))
    # the stages see the composite: a patch under an all-foreground mask is extract_aug's
    full = np.ones((4, 5), np.uint8)
    row = np.array([1.125, 0.75, 1.25, 0.0, 3, tr.AUG_HSV | tr.AUG_BLUR, 0, 0], np.float32)
    g = pr.geom_of(0, 0, 4, 3, 8)
    assert np.array_equal(bg.extract_aug_bg(frame, full, g, row, 0, 8, 1, 0, image),
                          tr.extract_aug(frame, g, row, 0, 8, 1, 0))
    assert not np.array_equal(bg.extract_aug_bg(frame, mask, g, row, 0, 8, 1, 0, image),
                              tr.extract_aug(frame, g, row, 0, 8, 1, 0))


# ------------------------------------------------------------------------------ plumbing
def test_header_signatures_and_library_agree_on_the_new_export():
    from scflow_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scflow_hip.h")).read(),
                 flags=re.S)
    lib = _lib.load()
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME) and not NAME.startswith("scflow_patch_")
    args = re.search(NAME + r"\s*\(([^)]*)\)", src).group(1)
    assert len(args.split(",")) == len(_lib.SIGNATURES[NAME][1]) == 28
    define = lambda n: int(re.search(rf"#define\s+SCFLOW_{n}\s+(\d+)", src).group(1))  # noqa: E731
    assert define("RNG_BACKGROUND") == _lib.RNG_BACKGROUND == bg.RNG_BACKGROUND == 3
    # what existing callers pin stays
    assert define("TRAIN_CFG_LEN") == len(_lib.TRAIN_CFG) == 20 and define("ABI_VERSION") == 4
    from scflow_amd import patches
    assert patches.TRAIN_AUG == tr.CFG


def test_argument_errors_are_codes_before_any_launch():
    from scflow_amd import _lib
    lib = _lib.load()
    one = 1  # any non-null address: the checks come before anything is dereferenced
    # frames, frame_index, geom, valid, aug, out, masks, pool, sizes, choice, chosen

    def ext(ptrs, slots=3, hb=24, wb=40, p=0.3, size=32):
        return getattr(lib, NAME)(*ptrs, 1, 1, 48, 64, size, 128, None, None, 0, slots, hb, wb, p,
                                  0, 0, 0, None)
    ok = [16] * 6 + [one, one, None, None, one]
    assert ext(ok[:6] + [None, one, None, None, one]) == -1   # masks
    assert ext(ok[:6] + [one, None, None, None, one]) == -1   # pool
    assert ext(ok[:6] + [one, one, None, None, None]) == -1   # chosen
    assert ext([None] + ok[1:]) == -1                         # what the plain entry refuses
    assert ext(ok, slots=0) == -1 and ext(ok, slots=-2) == -1
    assert ext(ok, hb=0) == -1 and ext(ok, wb=0) == -1
    for p in (-0.01, 1.01, float("nan"), float("inf")):
        assert ext(ok, p=p) == -1, p
    assert ext(ok, hb=(1 << 20) + 1) == -2 and ext(ok, wb=(1 << 20) + 1) == -2
    assert ext(ok, size=30) == -2
    assert ext(ok[:5] + [8] + ok[6:]) == -3                   # out's alignment, as the plain entry


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


@pytest.mark.parametrize("n", [5, 0])
def test_fake_implementation_gives_shapes_and_dtypes(n):
    from scflow_amd import library  # noqa: F401  (registers the ops)
    i32, u8 = torch.int32, torch.uint8
    for sizes, index in ((None, None), (_meta(3, 2, dtype=i32), _meta(n, dtype=i32))):
        img, chosen = torch.ops.scflow.patch_extract_aug_bg(
            _meta(2, 48, 64, 3, dtype=u8), _meta(2, 48, 64, dtype=u8), _meta(n, dtype=i32),
            _meta(n, 8, dtype=i32), _meta(n, dtype=u8), _meta(n, 8), _meta(3, 24, 40, 3, dtype=u8),
            sizes, index, 0.3, 32, 1, 0, 0, 128, None, None, True, True)
        assert tuple(img.shape) == (n, 3, 32, 32) and img.dtype == torch.float32
        assert tuple(chosen.shape) == (n,) and chosen.dtype == i32


def test_ops_and_patches_refuse_before_device_work():
    from scflow_amd import ops, patches
    from scflow_amd._lib import ScflowError
    i32, u8 = torch.int32, torch.uint8
    frames, masks = torch.zeros(2, 48, 64, 3, dtype=u8), torch.zeros(2, 48, 64, dtype=u8)
    lab, geom, valid = torch.zeros(2, dtype=i32), torch.zeros(2, 8, dtype=i32), torch.ones(2, dtype=u8)
    aug, pool = torch.zeros(2, 8), torch.zeros(3, 24, 40, 3, dtype=u8)
    call = lambda pool=pool, **kw: ops.extract_patches_aug_bg(  # noqa: E731
        frames, masks, lab, geom, valid, aug, pool, 32, 1, 0, **kw)
    with pytest.raises(ScflowError, match="is on cpu"):
        call()
    with pytest.raises(ScflowError, match="uint8"):
        call(pool=pool.float())
    with pytest.raises(ScflowError, match="uint8"):
        call(pool=pool[..., :2])
    with pytest.raises(ScflowError, match=r"background_sizes\[1\]"):
        call(background_sizes=torch.tensor([[24, 40], [25, 40], [5, 2]], dtype=i32))
    with pytest.raises(ScflowError, match=r"background_sizes\[2\]"):
        call(background_sizes=torch.tensor([[24, 40], [17, 33], [5, 0]], dtype=i32))
    with pytest.raises(ScflowError, match=r"\[3, 2\]"):
        call(background_sizes=torch.tensor([[24, 40]], dtype=i32))
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(ScflowError, match="probability"):
            call(p=p)
    R, t, pts = torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3), torch.zeros(3, 64, 3)
    cnt, diam = torch.full((3,), 64, dtype=i32), torch.ones(3)
    train = lambda **kw: patches.frames_to_train_patches(  # noqa: E731
        frames, masks, lab, R, t, R, lab, pts, cnt, diam, 1, 0, size=32, **kw)
    with pytest.raises(ScflowError, match="is on cpu"):
        train(backgrounds=pool)
    with pytest.raises(TypeError):  # keyword-only
        patches.frames_to_train_patches(frames, masks, lab, R, t, R, lab, pts, cnt, diam, 1, 0, None,
                                        32, 0, 32, 128, None, True, pool)
