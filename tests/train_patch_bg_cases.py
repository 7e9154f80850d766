"""The shapes the background tests share (tests/test_train_patch_bg_host.py on the CPU,
tests/test_gpu_train_patch_bg_ops.py on the GPU): F = 2 frames of 48 × 64, S = 32, a pool of B = 3
slots of 24 × 40 whose used sizes are (24, 40), (17, 33) and (5, 2), and the eight boxes of
tests/test_gpu_train_patch_ops.py — its six valid ones, the two-pixel-wide one and the invalid one
— plus its object whose frame index lies outside the frames (the first box again)."""
from functools import lru_cache

import numpy as np

from tests import patch_restatement as pr

S, H, W = 32, 48, 64
SLOTS, HB, WB = 3, 24, 40
SIZES = [(24, 40), (17, 33), (5, 2)]
BOXES = [(10, 5, 29, 24),      # inside the frame, upscale (crop 20)
         (8, 1, 52, 45),       # inside, downscale (crop 45)
         (30, 20, 45, 35),     # inside, exact 2× (crop 16)
         (-7, -5, 13, 14),     # leaves the frame top-left (21 × 20)
         (40, 25, 80, 64),     # leaves it bottom-right (41 × 40)
         (-10, -20, 79, 69),   # larger than the frame (crop 90)
         (20, 10, 21, 30),     # two pixels wide: the blur folds −2 … 3 onto 0, 1
         (0, 0, 0, 0),         # invalid
         (10, 5, 29, 24)]      # valid flag set, frame index outside the frames
FRAME_INDEX = [0, 1, 0, 1, 0, 1, 1, 1, 7]
VALID = [1, 1, 1, 1, 1, 1, 1, 0, 1]
INSIDE = [0, 1, 2, 6]          # crops that do not leave the frame
LEAVING = [3, 4, 5]            # crops with pad pixels
LIVE = [i for i, (v, f) in enumerate(zip(VALID, FRAME_INDEX)) if v and f < 2]


def geoms(size=S):
    return np.array([pr.geom_of(*b, size) if v else (0,) * 8 for b, v in zip(BOXES, VALID)], np.int32)


@lru_cache(maxsize=None)
def case():
    """frames [2, H, W, 3], a random mask, a checkerboard of 3 × 3 cells, the pool and its sizes."""
    from scflow_amd import synthetic
    rng = np.random.default_rng(23)
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    mask = ((rng.random((2, H, W)) > 0.5) * rng.integers(1, 256, (2, H, W))).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    cell = (yy // 3 + xx // 3) % 2
    checker = np.stack([cell * 255, (1 - cell) * 7]).astype(np.uint8)  # any nonzero byte is foreground
    # every slot is filled to its edges, so a read past a used size would show
    pool, _ = synthetic.make_background_pool(SLOTS, HB, WB, seed=5, full=True)
    out = dict(frames=frames, mask=mask, checker=checker, pool=pool,
               sizes=np.array(SIZES, np.int32), zeros=np.zeros((2, H, W), np.uint8),
               ones=np.full((2, H, W), 1, np.uint8))
    for v in out.values():
        v.setflags(write=False)
    return out
