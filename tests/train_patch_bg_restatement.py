"""NumPy restatement of the background stage of the training-patch contract (DESIGN.md §18,
include/scflow_hip.h scflow_train_patch_extract_bg; the reference's RandomBackground,
color_transform.py:177-244): the draw, the background resized to the crop's own size, and the
select under the instance mask, stage by stage on the crop array.  The generator, the colour stages
and the finish come from tests/train_patch_restatement.py, the coordinates and the resample from
tests/patch_restatement.py.

``dtype=np.float32`` performs every floating-point operation in fp32, one rounding per operation in
the contract's order (what the kernel computes); ``dtype=np.float64`` is the same definition in
fp64.  The select and the mask have one form.
"""
import numpy as np

from tests import patch_restatement as pr
from tests.train_patch_restatement import augment, finish, u01, words

RNG_BACKGROUND = 3


def draw(obj, seed, step, p, slots, dtype=np.float32):
    """The slot object ``obj`` takes, −1 for none: word 0 of (0, obj, BACKGROUND) decides
    (u ≤ p), word 1 picks min(int(u·slots), slots − 1)."""
    w = words(0, obj, RNG_BACKGROUND, seed, step)
    if not u01(w[0], dtype) <= dtype(np.float32(p)):
        return -1
    return min(int(dtype(u01(w[1], dtype) * dtype(slots))), slots - 1)


def chosen(index, slots, sizes=None, shape=None):
    """What an override entry becomes: itself in [0, slots), else −1; −1 also where the slot's
    sizes row is no used size of a ``shape`` = (Hb, Wb) slot."""
    b = int(index) if 0 <= int(index) < slots else -1
    if b >= 0 and sizes is not None:
        h, w = (int(v) for v in sizes[b])
        if not (1 <= h <= shape[0] and 1 <= w <= shape[1]):
            b = -1
    return b


def used(pool, sizes, slot):
    """The used region of a slot: top-left aligned, sizes[slot] = (h, w); all of it without sizes."""
    if sizes is None:
        return pool[slot]
    h, w = (int(v) for v in sizes[slot])
    return pool[slot][:h, :w]


def background_crop(image, cw, ch, dtype=np.float32):
    """cv2.resize(image, (cw, ch), INTER_LINEAR) as the contract defines it, aspect ratio not kept:
    the §15 resample of the used region, rounded to a level → [ch, cw, 3] uint8."""
    return np.rint(pr.resize_linear(image, cw, ch, dtype)).astype(np.uint8)


def foreground(mask, x1, y1, x2, y2):
    """[ch, cw] bool: the crop pixel lies inside the frame and its mask byte is not 0 (Crop pads
    the mask with 0)."""
    return pr.crop(mask[..., None], x1, y1, x2, y2, 0, np.uint8)[..., 0] != 0


def composite(crop, fg, bg):
    """merge_background_by_mask (mask.py:382-386): alpha is 0 or 1, a select."""
    return np.where(fg[..., None], crop, bg)


def composite_crop(frame, mask, geom, image, pad=128, dtype=np.float32):
    """The uint8 crop [ch, cw, 3] the colour stages see under a background ``image`` (None: the
    plain crop)."""
    x1, y1, x2, y2 = (int(v) for v in geom[:4])
    crop = pr.crop(frame, x1, y1, x2, y2, pad, np.uint8)
    if image is None:
        return crop
    bg = background_crop(image, x2 - x1 + 1, y2 - y1 + 1, dtype)
    return composite(crop, foreground(mask, x1, y1, x2, y2), bg)


def extract_aug_bg(frame, mask, geom, row, obj, S, seed, step, image, dtype=np.float32, pad=128, **kw):
    """One valid object's patch [3, S, S]: crop, background select, stages, resize, pad,
    normalise."""
    crop = composite_crop(frame, mask, geom, image, pad, dtype)
    return finish(augment(crop, row, obj, seed, step, dtype), geom, S, pad=pad, dtype=dtype, **kw)
