"""GPU: scflow_train_patch_extract_bg (``ops.extract_patches_aug_bg``) against the NumPy restatement
of the contract (tests/train_patch_bg_restatement.py) and against the kernel without
a background (``ops.extract_patches_aug``).

Shapes: tests/train_patch_bg_cases.py — F = 2 frames of 48 × 64, S = 32, a pool of 3 slots of
24 × 40 with used sizes (24, 40), (17, 33), (5, 2), nine objects on eight boxes; one case at
S = 128 (two column tiles).  Bounds:

* no background chosen, or a mask that is foreground everywhere: ``extract_patches_aug``'s bits;
* background only, background + HSV + blur: integer levels equal to the fp32 restatement; the
  background alone within one level of the fp64 restatement, at most 0.5 % of the levels differing
  (tests/test_train_patch_bg_host.py holds the two restatements to that on the CPU);
* the select: an output pixel whose four taps are foreground is ``extract_patches_aug``'s, one
  whose four taps are background is the background-only run's, bit for bit;
* noise on the composite, as tests/test_gpu_train_patch_ops.py bounds it: at identity geometry
  equal to the fp64 restatement wherever its value before truncation lies more than 1e-3 from an
  integer (at most 1 % of the values may be that close), within one level elsewhere; and the whole
  chain exact from the device's own composite + HSV + noise crop;
* LDS-staged and direct routes: the same bits;
* the draw: the restatement's slots, whatever S, the tiling or geom[4:8].
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import patch_restatement as pr
from tests import train_patch_bg_cases as cs
from tests import train_patch_bg_restatement as bg
from tests import train_patch_restatement as tr
from tests.test_gpu_patch_ops import dev

pytestmark = pytest.mark.gpu

S = cs.S
SEED, STEP = 0x5CF10A3D2B17, 5
HSV, NOISE, BLUR = tr.AUG_HSV, tr.AUG_NOISE, tr.AUG_BLUR
N = len(cs.BOXES)
GAINS = [(1.125, 0.75, 1.25), (0.875, 1.375, 0.625), (1.0, 1.0, 1.0), (1.1875, 1.5, 1.5),
         (0.8125, 0.5, 0.875)]  # a short mantissa: level · gain is exact in fp32 and fp64


def rows_of(mask, ksize=1, sigma=0.07, n=N):
    return np.array([GAINS[i % len(GAINS)] + (sigma, ksize, mask, 0, 0) for i in range(n)], np.float32)


@lru_cache(maxsize=None)
def gpu():
    c = cs.case()
    out = {k: dev(v.copy()) for k, v in c.items()}  # the shared arrays are read-only
    out.update(fidx=dev(cs.FRAME_INDEX, torch.int32), valid=dev(cs.VALID, torch.uint8))
    return out


def run(rows, mask="mask", size=S, index=None, sizes=True, **kw):
    """(levels [N, 3, size, size], chosen [N]) of the nine objects; ``index``: one slot for all, a
    list, or None for the draw."""
    from scflow_amd import ops
    g = gpu()
    if index is not None:
        index = dev(np.full(N, index) if np.isscalar(index) else index, torch.int32)
    kw.setdefault("p", 1.0)
    img, chosen = ops.extract_patches_aug_bg(
        g["frames"], g[mask], g["fidx"], dev(cs.geoms(size)), g["valid"], dev(rows), g["pool"], size,
        SEED, STEP, background_sizes=g["sizes"] if sizes else None, background_index=index, **kw)
    return img, chosen.cpu().numpy()


def parent(rows, size=S, **kw):
    from scflow_amd import ops
    g = gpu()
    return ops.extract_patches_aug(g["frames"], g["fidx"], dev(cs.geoms(size)), g["valid"], dev(rows),
                                   size, SEED, STEP, **kw)


def levels(t):
    a = t.cpu().numpy()
    assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= 255
    return a


def restate(rows, slot, mask, dtype, size=S):
    """The nine patches under slot ``slot`` for every object; a pad patch for the two dead ones."""
    c = cs.case()
    image = bg.used(c["pool"], c["sizes"], slot)
    out = np.full((N, 3, size, size), 128, dtype)
    for i in cs.LIVE:
        f = cs.FRAME_INDEX[i]
        out[i] = bg.extract_aug_bg(c["frames"][f], c[mask][f], cs.geoms(size)[i], rows[i], i, size,
                                   SEED, STEP, image, dtype)
    return out


# ------------------------------------------------------------------------------ no background
@pytest.mark.parametrize("mask,ksize", [(0, 1), (HSV | NOISE | BLUR, 5)])
def test_no_background_chosen_is_the_kernel_without_one(mask, ksize):
    rows = rows_of(mask, ksize)
    want = parent(rows)
    got, chosen = run(rows, p=0.0)
    assert torch.equal(got, want) and (chosen == -1).all()
    got, chosen = run(rows, index=-1)
    assert torch.equal(got, want) and (chosen == -1).all()
    got, _ = run(rows, index=-1, direct=True)
    assert torch.equal(got, want)
    assert want[cs.LIVE].std() > 0


@pytest.mark.parametrize("mask,ksize", [(0, 1), (HSV | NOISE | BLUR, 5)])
def test_an_all_foreground_mask_is_the_kernel_without_one(mask, ksize):
    rows = rows_of(mask, ksize)
    want = parent(rows)
    got, chosen = run(rows, mask="ones")
    assert (chosen >= 0).all()  # a background was drawn, and nothing of it shows inside the frame
    assert torch.equal(got[cs.INSIDE], want[cs.INSIDE])
    assert not torch.equal(got[cs.LEAVING], want[cs.LEAVING])  # pad pixels are background
    dead = [i for i in range(N) if i not in cs.LIVE]
    assert torch.equal(got[dead], want[dead]) and (got[dead] == 128).all()


# ------------------------------------------------------------------------------ background only
@pytest.mark.parametrize("slot", range(cs.SLOTS))
def test_background_only_equals_the_fp32_restatement(slot):
    rows = rows_of(0)
    img, chosen = run(rows, mask="zeros", index=slot)
    got = levels(img)
    assert (chosen == slot).all()
    assert np.array_equal(got, levels(run(rows, mask="zeros", index=slot, direct=True)[0]))
    want32, want64 = (restate(rows, slot, "zeros", d) for d in (np.float32, np.float64))
    differ = (got != want64)[cs.LIVE].mean()
    print(f"slot {slot} {cs.SIZES[slot]}: {(got != want32).sum()} levels differ from the fp32 "
          f"restatement, {differ:.3%} from the fp64 one (by up to {np.abs(got - want64).max():.0f})")
    assert np.array_equal(got, want32)
    assert np.abs(got - want64).max() <= 1 and differ <= 0.005
    assert not np.array_equal(got[cs.LIVE], levels(parent(rows))[cs.LIVE])
    # nothing of the frame is left: the same patches from other frames
    from scflow_amd import ops
    g = gpu()
    other, _ = ops.extract_patches_aug_bg(
        g["frames"].flip(0).contiguous(), g["zeros"], g["fidx"], dev(cs.geoms()), g["valid"],
        dev(rows), g["pool"], S, SEED, STEP, p=1.0, background_sizes=g["sizes"],
        background_index=dev(np.full(N, slot), torch.int32))
    assert torch.equal(other, img)


def test_whole_slots_without_a_sizes_table():
    rows = rows_of(0)
    got = levels(run(rows, mask="zeros", index=1, sizes=False)[0])
    c = cs.case()
    for i in cs.LIVE:
        want = bg.extract_aug_bg(c["frames"][0], c["zeros"][0], cs.geoms()[i], rows[i], i, S, SEED,
                                 STEP, c["pool"][1])
        assert np.array_equal(got[i], want), i


# ------------------------------------------------------------------------------ the select
def _taps(i):
    """[4, nh, nw] crop pixel indices (y, x) of the four taps of every resized pixel of object i."""
    x1, y1, x2, y2, nw, nh, left, top = (int(v) for v in cs.geoms()[i])
    xa, xb, _ = pr.linear_coords(x2 - x1 + 1, nw)
    ya, yb, _ = pr.linear_coords(y2 - y1 + 1, nh)
    return [(y[:, None], x[None, :]) for y in (ya, yb) for x in (xa, xb)], (nw, nh, left, top)


def test_select_is_exact_under_a_checkerboard_mask():
    rows = rows_of(0)
    c = cs.case()
    plain, only = levels(parent(rows)), levels(run(rows, mask="zeros", index=0)[0])
    got = levels(run(rows, mask="checker", index=0)[0])
    assert np.array_equal(got, levels(run(rows, mask="checker", index=0, direct=True)[0]))
    assert np.array_equal(got, restate(rows, 0, "checker", np.float32))
    for i in cs.LEAVING + [0, 1]:
        fg = bg.foreground(c["checker"][cs.FRAME_INDEX[i]], *cs.BOXES[i])
        taps, (nw, nh, left, top) = _taps(i)
        n_fg = sum(fg[y, x].astype(int) for y, x in taps)
        inner = got[i][:, top:top + nh, left:left + nw]
        all_fg, all_bg = n_fg == 4, n_fg == 0
        print(f"object {i}: {all_fg.mean():.1%} of the resized pixels read foreground only, "
              f"{all_bg.mean():.1%} background only")
        assert all_fg.sum() >= 8 and all_bg.sum() >= 8 and (n_fg % 4 != 0).any()
        assert np.array_equal(inner[:, all_fg], plain[i][:, top:top + nh, left:left + nw][:, all_fg])
        assert np.array_equal(inner[:, all_bg], only[i][:, top:top + nh, left:left + nw][:, all_bg])


# ------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("ksize", [3, 5])
def test_background_hsv_and_blur_equal_the_fp32_restatement(ksize):
    rows = rows_of(HSV | BLUR, ksize)
    index = [i % cs.SLOTS for i in range(N)]
    got = levels(run(rows, index=index)[0])
    assert np.array_equal(got, levels(run(rows, index=index, direct=True)[0]))
    per_slot = [restate(rows, b, "mask", np.float32) for b in range(cs.SLOTS)]
    want = np.stack([per_slot[index[i]][i] for i in range(N)])
    assert np.array_equal(got, want)
    assert not np.array_equal(got, levels(run(rows_of(BLUR, ksize), index=index)[0]))
    assert not np.array_equal(got[cs.LIVE], levels(parent(rows))[cs.LIVE])


def _identity(box):
    side = box[2] - box[0] + 1
    assert side == box[3] - box[1] + 1 and side % 4 == 0
    g = pr.geom_of(*box, side)
    assert g[4:] == (side, side, 0, 0)
    return side, g


def _own(box, fi, row, slot, offset):
    """One object at identity geometry: every output pixel IS a crop pixel of the composite."""
    from scflow_amd import ops
    g = gpu()
    side, geom = _identity(box)
    img, _ = ops.extract_patches_aug_bg(
        g["frames"], g["mask"], dev([fi], torch.int32), dev(np.array([geom], np.int32)),
        dev([1], torch.uint8), dev(row), g["pool"], side, SEED, STEP, offset, p=1.0,
        background_sizes=g["sizes"], background_index=dev([slot], torch.int32))
    return levels(img)[0]


@pytest.mark.parametrize("box,fi,slot", [((10, 5, 29, 24), 0, 0), ((-7, -5, 12, 14), 1, 1),
                                         ((8, 1, 51, 44), 1, 2)])
def test_noise_on_the_composite_at_identity_geometry(box, fi, slot):
    c = cs.case()
    side, geom = _identity(box)
    row = rows_of(NOISE, sigma=0.1, n=1)
    got = _own(box, fi, row, slot, 3)
    crop = bg.composite_crop(c["frames"][fi], c["mask"][fi], geom, bg.used(c["pool"], c["sizes"], slot))
    exact = tr.noise_values(crop, 0.1, 3, SEED, STEP, np.float64).transpose(2, 0, 1)
    want = np.clip(exact, 0, 255).astype(np.uint8)
    near = (np.abs(exact - np.rint(exact)) <= 1e-3) & (exact > -1e-3) & (exact < 255 + 1e-3)
    print(f"crop {side}: {near.mean():.3%} of the values within 1e-3 of an integer, "
          f"{(got != want).sum()} levels differ")
    assert near.mean() <= 0.01
    assert np.array_equal(got[~near], want[~near]) and np.abs(got - want).max() <= 1
    assert (got != crop.transpose(2, 0, 1)).mean() > 0.9


def test_full_chain_is_exact_on_the_devices_own_composite():
    """Composite + HSV + noise read back at identity geometry, then blur and resize restated: the
    S = 32 output of the same objects, bit for bit."""
    from scflow_amd import ops
    g = gpu()
    boxes, fidx, slots = [(10, 5, 29, 24), (8, 1, 51, 44), (30, 20, 45, 35)], [0, 1, 0], [2, 0, 1]
    geom = [pr.geom_of(*b, S) for b in boxes]
    for ksize in (3, 5):
        rows = rows_of(HSV | NOISE | BLUR, ksize, n=3)
        args = (g["frames"], g["mask"], dev(fidx, torch.int32), dev(np.array(geom, np.int32)),
                dev([1] * 3, torch.uint8), dev(rows), g["pool"], S, SEED, STEP)
        kw = dict(p=1.0, background_sizes=g["sizes"], background_index=dev(slots, torch.int32))
        full = levels(ops.extract_patches_aug_bg(*args, **kw)[0])
        assert np.array_equal(full, levels(ops.extract_patches_aug_bg(*args, direct=True, **kw)[0]))
        for i, b in enumerate(boxes):
            pre = rows[i:i + 1].copy()
            pre[0, 5] = HSV | NOISE
            crop = _own(b, fidx[i], pre, slots[i], i).transpose(1, 2, 0).astype(np.uint8)
            assert np.array_equal(full[i], tr.finish(tr.blur_stage(crop, ksize), geom[i], S)), (ksize, i)


def test_a_patch_side_with_two_column_tiles():
    """S = 128: a workgroup's tile is 16 × 64 output pixels, so every patch row is cut at column 64."""
    rows = rows_of(HSV | BLUR, 5)
    index = [(i + 1) % cs.SLOTS for i in range(N)]
    img, chosen = run(rows, size=128, index=index)
    got = levels(img)
    assert chosen.tolist() == index
    assert np.array_equal(got, levels(run(rows, size=128, index=index, direct=True)[0]))
    per_slot = [restate(rows, b, "mask", np.float32, 128) for b in range(cs.SLOTS)]
    assert np.array_equal(got, np.stack([per_slot[index[i]][i] for i in range(N)]))
    only = run(rows_of(0), mask="zeros", size=128, index=index)[0]
    assert torch.equal(only, run(rows_of(0), mask="zeros", size=128, index=index, direct=True)[0])
    noisy = run(rows_of(HSV | NOISE | BLUR, 5), size=128, index=index)[0]
    assert torch.equal(noisy, run(rows_of(HSV | NOISE | BLUR, 5), size=128, index=index, direct=True)[0])
    assert not np.array_equal(levels(noisy), got)


def test_a_slot_wide_enough_for_the_64_bit_coordinate():
    """(2x + 1)·w_b leaves 32 bits where 2·cw·w_b ≥ 2^31: a 4000-px crop (of a 16 × 4096 frame, no
    window of which fits the LDS budget) on a slot 2^19 wide; the 60-px crop next to it stays in 32
    bits on the same slot and is staged."""
    from scflow_amd import ops
    from tests.test_gpu_patch_ops import _wide_case
    frames, geom = _wide_case()
    wb = 1 << 19
    assert 2 * 4000 * wb >= 2 ** 31 > 2 * 60 * wb
    rng = np.random.default_rng(9)
    pool = rng.integers(0, 256, (1, 2, wb, 3), dtype=np.uint8)
    mask = (rng.random((1, 16, 4096)) > 0.5).astype(np.uint8)
    for stage in (0, HSV | BLUR):
        rows = rows_of(stage, 5, n=2)
        args = (dev(frames), dev(mask), dev([0, 0], torch.int32), dev(geom), dev([1, 1], torch.uint8),
                dev(rows), dev(pool), S, SEED, STEP)
        kw = dict(background_index=dev([0, 0], torch.int32))
        img, chosen = ops.extract_patches_aug_bg(*args, **kw)
        assert chosen.tolist() == [0, 0]
        assert torch.equal(img, ops.extract_patches_aug_bg(*args, direct=True, **kw)[0])
        want = np.stack([bg.extract_aug_bg(frames[0], mask[0], geom[i], rows[i], i, S, SEED, STEP, pool[0])
                         for i in range(2)])
        assert np.array_equal(levels(img), want)
        assert not np.array_equal(want, np.stack([tr.extract_aug(frames[0], geom[i], rows[i], i, S, SEED,
                                                                 STEP) for i in range(2)]))


# ------------------------------------------------------------------------------ the draw
N_DRAW, DRAW_OFFSET, P = 64, 5, 0.3


def _draw(size=S, offset=DRAW_OFFSET, geom=None, n=N_DRAW, first=0, **kw):
    from scflow_amd import ops
    g = gpu()
    if geom is None:
        geom = np.array([cs.geoms(size)[i % 7] for i in range(N_DRAW)], np.int32)
    sl = slice(first, first + n)
    kw.setdefault("p", P)
    kw.setdefault("background_sizes", g["sizes"])
    return ops.extract_patches_aug_bg(
        g["frames"], g["mask"], dev((np.arange(N_DRAW) % 2)[sl], torch.int32), dev(geom[sl]),
        dev(np.ones(N_DRAW, np.uint8)[sl]), dev(rows_of(HSV, n=N_DRAW)[sl]), g["pool"], size, SEED,
        STEP, offset, **kw)[1].cpu().numpy()


def test_chosen_slots_equal_the_restatement():
    want = [bg.draw(DRAW_OFFSET + i, SEED, STEP, P, cs.SLOTS) for i in range(N_DRAW)]
    got = _draw()
    print(f"{(got >= 0).sum()} of {N_DRAW} objects take a background: slots "
          f"{np.bincount(got[got >= 0]).tolist()}")
    assert got.tolist() == want and -1 in want and set(want) >= {0, 1, 2}
    assert (_draw(p=1.0) >= 0).all() and (_draw(p=0.0) == -1).all()
    # neither the patch side (one tile at 32, sixteen at 128), the route, nor nw, nh, left, top
    assert np.array_equal(_draw(size=128), got) and np.array_equal(_draw(direct=True), got)
    geom = np.array([cs.geoms()[i % 7] for i in range(N_DRAW)], np.int32)
    geom[:, 4:6], geom[:, 6:8] = 8, 3
    assert np.array_equal(_draw(geom=geom), got)
    # an invalid object draws all the same
    geom[:] = 0
    assert np.array_equal(_draw(geom=geom), got)


def test_chosen_slots_shift_with_object_offset():
    full, k = _draw(), 9
    assert np.array_equal(_draw(offset=DRAW_OFFSET + k, n=N_DRAW - k, first=k), full[k:])
    assert np.array_equal(_draw(offset=DRAW_OFFSET + k)[:-k], full[k:])
    assert not np.array_equal(_draw(offset=DRAW_OFFSET + 1), full)


def test_override_is_honoured():
    index = np.array([(-1, 0, 1, 2, 3, -2, 99, 2)[i % 8] for i in range(N_DRAW)], np.int32)
    want = [bg.chosen(v, cs.SLOTS) for v in index]
    assert _draw(background_index=dev(index), p=0.0).tolist() == want
    assert _draw(background_index=dev(index), p=1.0).tolist() == want
    # a device sizes table is taken as it is: a row that is no used size leaves its objects without
    sizes = np.array([(24, 40), (25, 40), (5, 0)], np.int32)
    want = [bg.chosen(v, cs.SLOTS, sizes, (cs.HB, cs.WB)) for v in index]
    assert set(want) == {-1, 0}
    assert _draw(background_index=dev(index), background_sizes=dev(sizes)).tolist() == want
    rows = rows_of(HSV | BLUR, 3)
    from scflow_amd import ops
    g = gpu()
    img, chosen = ops.extract_patches_aug_bg(
        g["frames"], g["mask"], g["fidx"], dev(cs.geoms()), g["valid"], dev(rows), g["pool"], S, SEED,
        STEP, p=1.0, background_sizes=dev(sizes), background_index=dev(np.full(N, 1), torch.int32))
    assert (chosen.cpu().numpy() == -1).all() and torch.equal(img, parent(rows))


# ------------------------------------------------------------------------------ plumbing
def _call():
    from scflow_amd import ops
    g = gpu()
    rows, geom = dev(rows_of(HSV | NOISE | BLUR, 3)), dev(cs.geoms())

    def go():
        return ops.extract_patches_aug_bg(g["frames"], g["mask"], g["fidx"], geom, g["valid"], rows,
                                          g["pool"], S, SEED, STEP, p=0.5,
                                          background_sizes=g["sizes"])
    return go


def test_runs_on_the_current_stream():
    go = _call()
    want = go()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = go()
    s.synchronize()
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    assert (want[1] >= 0).any() and (want[1] == -1).any()


def test_graph_capture_and_replay():
    go = _call()
    eager = go()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        go()  # allocator warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = go()
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager[0], out[0]) and torch.equal(eager[1], out[1])


def test_no_objects_and_refusals():
    from scflow_amd import ops
    from scflow_amd._lib import ScflowError
    g = gpu()
    e = lambda *s, dt=torch.float32: torch.empty(*s, device="cuda", dtype=dt)  # noqa: E731
    img, chosen = ops.extract_patches_aug_bg(g["frames"], g["mask"], e(0, dt=torch.int32),
                                             e(0, 8, dt=torch.int32), e(0, dt=torch.uint8), e(0, 8),
                                             g["pool"], S, 1, 0)
    assert tuple(img.shape) == (0, 3, S, S) and tuple(chosen.shape) == (0,) and chosen.dtype == torch.int32
    rows, geom = dev(rows_of(0)), dev(cs.geoms())
    call = lambda *a, **kw: ops.extract_patches_aug_bg(  # noqa: E731
        g["frames"], a[0] if a else g["mask"], g["fidx"], geom, g["valid"], rows,
        kw.pop("pool", g["pool"]), S, 1, 0, **kw)
    with pytest.raises(ScflowError, match=r"masks must be \[2, 48, 64\]"):
        call(g["mask"][:, :40].contiguous())
    with pytest.raises(ScflowError, match="is on cpu"):
        call(pool=g["pool"].cpu())
    with pytest.raises(ScflowError, match=r"background_index must be \[9\]"):
        call(background_index=dev([0, 1], torch.int32))
    with pytest.raises(ScflowError, match=r"background_sizes\[1\]"):
        call(background_sizes=torch.tensor([[24, 40], [24, 41], [5, 2]], dtype=torch.int32))
    # a host table is checked, then copied: the same result as the device table
    a = call(background_sizes=torch.tensor(cs.SIZES, dtype=torch.int32), p=1.0)
    b = call(background_sizes=g["sizes"], p=1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_opcheck():
    from scflow_amd import library  # noqa: F401  (registers the ops)
    g = gpu()
    rows = dev(rows_of(HSV | NOISE | BLUR, 3))
    index = dev(np.arange(N) % 4 - 1, torch.int32)
    for sizes, idx in ((g["sizes"], index), (None, None)):
        args = (g["frames"], g["mask"], g["fidx"], dev(cs.geoms()), g["valid"], rows, g["pool"], sizes,
                idx, 0.5, S, SEED, STEP, 0, 128, [10.0, 20.0, 30.0], [58.395, 57.12, 57.375], True, True)
        torch.library.opcheck(torch.ops.scflow.patch_extract_aug_bg.default, args)
    from scflow_amd import ops
    want = ops.extract_patches_aug_bg(g["frames"], g["mask"], g["fidx"], dev(cs.geoms()), g["valid"],
                                      rows, g["pool"], S, SEED, STEP, 0, 0.5, None, None, 128,
                                      [10.0, 20.0, 30.0], [58.395, 57.12, 57.375], True, True)
    got = torch.ops.scflow.patch_extract_aug_bg(*args)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
