"""Timing of the patch path: scflow_patch_boxes + scflow_patch_extract next to the
per-object PyTorch loop, on the device, alternating in one process.

usage: python tools/patch_bench.py [--frames 4] [--height 480] [--width 640] [--objects 32]
                                   [--size 256] [--rounds 9] [--steps 50] [--json out.json]

The scene: `frames` seeded random uint8 frames, `objects` ellipsoid-sized point clouds posed in
front of a YCB-V-like camera (seeded; the crop sizes are printed), ratio 1.1.  Timed, each window
between two device events around `steps` calls, after a warm-up of every shape:

* `hip`: the two launches (`ops.patch_boxes`, `ops.extract_patches`) — and `hip_staged`, the same
  with SCFLOW_PATCH_LDS=1 (source rows staged in LDS instead of every tap read from global memory);
* `torch_loop`: tests/patch_restatement.py `torch_patches` on the geometry the box kernel
  produced — pad, slice, one `interpolate` per object, after `geom.tolist()`, its host
  synchronisation.  It does not include the projection and box arithmetic, so the ratio favours it.

Prints the medians, the ratio, the bytes the extract launch has to move (from the shapes) and one
JSON line.  No threshold: the parent has no such path.

`--train` times the training front end instead, alternating in the same way:

* `plain`: the two launches above at the GT pose (what inference runs);
* `train`: `ops.train_draw` + `ops.patch_boxes` at the jittered pose with the drawn ratio +
  `ops.extract_patches_aug` with the config's augmentation (`patches.TRAIN_AUG`: every stage on);
* `train_direct`: the same with the extract's direct route forced (every tap computes its own
  window; the same bits);
* `train_mask0`: the same three launches with every stage probability below 0 (stage mask 0: the
  extract does `plain`'s work).

`--train --background` adds the background stage to the same alternation:

* `train_bg_p03`, `train_bg_p1`: `train` with `ops.extract_patches_aug_bg` in place of the extract,
  a pool of `--slots` (64) seeded slots of `--pool-height` × `--pool-width` (480 × 640) used in
  full, at p = 0.3 and p = 1.  The instance masks are the ellipses inscribed in the objects' boxes
  at the GT pose.  Also printed: the bytes the stage adds at p = 1, from the shapes — one mask byte
  per crop pixel inside the frame and 12 pool bytes per background pixel of a crop.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(a, dev):
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (a.frames, a.height, a.width, 3), dtype=np.uint8))
    points = rng.uniform(-1.0, 1.0, (21, 1000, 3)).astype(np.float32)
    points *= rng.uniform(45.0, 135.0, (21, 1, 1)).astype(np.float32) * np.array([1.0, 0.76, 0.6], np.float32)
    K = np.array([[1066.8, 0, 312.99], [0, 1067.5, 241.31], [0, 0, 1]], np.float32)
    Rs, ts = [], []
    for _ in range(a.objects):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        Rs.append(q * np.sign(np.linalg.det(q)))
        tz = rng.uniform(700.0, 1300.0)
        ts.append([rng.uniform(-0.22, 0.22) * tz, rng.uniform(-0.16, 0.16) * tz, tz])
    T = lambda x, dt=torch.float32: torch.as_tensor(np.asarray(x)).to(dt).to(dev)  # noqa: E731
    return dict(frames=frames.to(dev), points=T(points), counts=T(np.full(21, 1000), torch.int32),
                labels=T(rng.integers(0, 21, a.objects), torch.int32), R=T(np.stack(Rs)), t=T(ts),
                K=T(np.repeat(K[None], a.frames, 0)),
                fidx=T(rng.integers(0, a.frames, a.objects), torch.int32),
                ratio=torch.full((a.objects,), 1.1, device=dev))


def train_bench(a, s):
    """The `--train` mode: see the module docstring."""
    from scflow_amd import ops, patches
    dev = s["frames"].device
    norm = dict(mean=[0.0] * 3, std=[255.0] * 3, to_rgb=True)
    diam = torch.full((21,), 180.0, device=dev)
    off = dict(patches.TRAIN_AUG, p_hsv=-1.0, p_noise=-1.0, p_blur=-1.0)
    seed = 2024

    def boxes(R, t, ratio):
        return ops.patch_boxes(s["points"], s["counts"], s["labels"], R, t, s["K"], ratio, a.height,
                               a.width, a.size, frame_index=s["fidx"], num_frames=a.frames,
                               k_per_frame=True)

    def plain():
        _, geom, _, _, valid = boxes(s["R"], s["t"], s["ratio"])
        return ops.extract_patches(s["frames"], s["fidx"], geom, valid, a.size, pad=128.0, **norm)

    def train(cfg=patches.TRAIN_AUG, direct=False, step=0):
        R, t, _, ok, tries, ratio, rows = ops.train_draw(s["points"], s["counts"], s["labels"], diam,
                                                         s["R"], s["t"], cfg, seed, step)
        _, geom, _, _, valid = boxes(R, t, ratio)
        img = ops.extract_patches_aug(s["frames"], s["fidx"], geom, valid, rows, a.size, seed, step,
                                      direct=direct, **norm)
        return img, ok, tries, rows, geom, valid

    run = {"plain": plain, "train": train, "train_direct": lambda: train(direct=True),
           "train_mask0": lambda: train(cfg=off)}
    if a.background:
        from scflow_amd import synthetic
        pool = torch.from_numpy(synthetic.make_background_pool(a.slots, a.pool_height, a.pool_width,
                                                               full=True)[0]).to(dev)
        masks = ellipse_masks(a, s, boxes(s["R"], s["t"], torch.ones_like(s["ratio"]))[0])

        def train_bg(p, step=0):
            R, t, _, ok, tries, ratio, rows = ops.train_draw(s["points"], s["counts"], s["labels"],
                                                             diam, s["R"], s["t"],
                                                             patches.TRAIN_AUG, seed, step)
            _, geom, _, _, valid = boxes(R, t, ratio)
            return ops.extract_patches_aug_bg(s["frames"], masks, s["fidx"], geom, valid, rows, pool,
                                              a.size, seed, step, p=p, **norm) + (geom, valid)

        run["train_bg_p03"], run["train_bg_p1"] = (lambda: train_bg(0.3)), (lambda: train_bg(1.0))
    outs = {}
    for k, f in run.items():
        for _ in range(3):
            outs[k] = f()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, f in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.steps)
    img, ok, tries, rows, geom, valid = outs["train"]
    g = geom.cpu().numpy()
    cw = (g[:, 2] - g[:, 0] + 1)[valid.cpu().numpy() != 0]
    res = dict(mode="train", frames=a.frames, height=a.height, width=a.width, objects=a.objects,
               size=a.size, rounds=a.rounds, steps=a.steps, valid=int(valid.sum()),
               accepted=int(ok.sum()), max_tries=int(tries.max()), crop_min=int(cw.min()),
               crop_max=int(cw.max()), ksizes=sorted(set(rows[:, 4].tolist())),
               same_bits_tiled_direct=bool(torch.equal(img, outs["train_direct"][0])))
    for k, v in times.items():
        res[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
        print(f"{k}: median {res[k]['median_ms']:.4f} ms/call (min {min(v):.4f}, max {max(v):.4f})")
    res["train_over_plain"] = res["train"]["median_ms"] / res["plain"]["median_ms"]
    if a.background:
        _, c03, _, _ = outs["train_bg_p03"]
        _, c1, geom1, valid1 = outs["train_bg_p1"]
        inside, bgpx = background_bytes(a, s, masks, geom1, valid1)
        res.update(slots=a.slots, pool_height=a.pool_height, pool_width=a.pool_width,
                   replaced_p03=int((c03 >= 0).sum()), replaced_p1=int((c1 >= 0).sum()),
                   mask_bytes_p1=inside, pool_bytes_p1=12 * bgpx,
                   same_bits_p0_train=bool(torch.equal(
                       img, ops.extract_patches_aug_bg(s["frames"], masks, s["fidx"], geom, valid,
                                                       rows, pool, a.size, seed, 0, p=0.0, **norm)[0])))
        print(f"background: {a.slots} slots of {a.pool_height}×{a.pool_width}; p = 0.3 replaces "
              f"{res['replaced_p03']} of {a.objects} objects, p = 1 {res['replaced_p1']}; at p = 1 the "
              f"stage reads {inside / 1e6:.2f} MB of mask (one byte per crop pixel inside the frame) "
              f"and up to {12 * bgpx / 1e6:.2f} MB of pool (12 B per background pixel of a crop), "
              f"before the halo and the overlap of neighbouring tiles' windows; p = 0 "
              f"{'equals' if res['same_bits_p0_train'] else 'DIFFERS FROM'} `train` bit for bit")
    print(f"F={a.frames} frames of {a.height}×{a.width}, N={a.objects} objects ({res['valid']} valid, "
          f"{res['accepted']} jittered within {res['max_tries']} tries, crops {res['crop_min']}-"
          f"{res['crop_max']} px), S={a.size}: train / plain = {res['train_over_plain']:.2f}×; tiled "
          f"and direct routes {'equal' if res['same_bits_tiled_direct'] else 'DIFFER'} bit for bit")
    return res


def ellipse_masks(a, s, bbox):
    """[F, H, W] uint8 instance masks: the ellipse inscribed in every object's box (l, t, r, b)."""
    yy, xx = np.mgrid[0:a.height, 0:a.width]
    masks = np.zeros((a.frames, a.height, a.width), np.uint8)
    for (l, t, r, b), f in zip(bbox.cpu().numpy().tolist(), s["fidx"].cpu().numpy().tolist()):
        if not np.isfinite([l, t, r, b]).all() or r <= l or b <= t:
            continue
        inside = ((xx - (l + r) / 2) / ((r - l) / 2)) ** 2 + ((yy - (t + b) / 2) / ((b - t) / 2)) ** 2 <= 1
        masks[f][inside] = 255
    return torch.from_numpy(masks).to(s["frames"].device)


def background_bytes(a, s, masks, geom, valid):
    """(crop pixels inside the frame, background pixels of the crops) over the valid objects."""
    m = masks.cpu().numpy()
    inside = bgpx = 0
    for (x1, y1, x2, y2, *_), f, v in zip(geom.cpu().numpy().tolist(), s["fidx"].cpu().numpy().tolist(),
                                          valid.cpu().numpy().tolist()):
        if not v:
            continue
        xa, xb, ya, yb = max(x1, 0), min(x2, a.width - 1), max(y1, 0), min(y2, a.height - 1)
        win = m[f][ya:yb + 1, xa:xb + 1]
        inside += win.size
        bgpx += (x2 - x1 + 1) * (y2 - y1 + 1) - int((win != 0).sum())
    return inside, bgpx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--objects", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--json", default=None)
    ap.add_argument("--train", action="store_true", help="time the training front end (§17)")
    ap.add_argument("--background", action="store_true",
                    help="with --train: add the background stage at p = 0.3 and p = 1 (§18)")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--pool-height", type=int, default=480)
    ap.add_argument("--pool-width", type=int, default=640)
    a = ap.parse_args()
    if a.background and not a.train:
        raise SystemExit("--background times the training front end: pass --train with it")
    if not torch.cuda.is_available():
        raise SystemExit("patch_bench needs a GPU: a CPU run says nothing about these timings")
    from scflow_amd import _lib, ops
    from tests.patch_restatement import torch_patches
    dev = torch.device("cuda")
    s = scene(a, dev)
    if a.train:
        write_json(a, train_bench(a, s))
        return
    norm = dict(pad=128.0, mean=[0.0] * 3, std=[255.0] * 3, to_rgb=True)

    def boxes():
        return ops.patch_boxes(s["points"], s["counts"], s["labels"], s["R"], s["t"], s["K"],
                               s["ratio"], a.height, a.width, a.size, frame_index=s["fidx"],
                               num_frames=a.frames, k_per_frame=True)

    def hip():
        _, geom, _, _, valid = boxes()
        return ops.extract_patches(s["frames"], s["fidx"], geom, valid, a.size, **norm)

    _, geom, _, _, valid = boxes()

    def loop():
        return torch_patches(s["frames"], s["fidx"], geom, valid, a.size, **norm)

    def set_lds(on):
        os.environ["SCFLOW_PATCH_LDS"] = "1" if on else "0"
        _lib.reload_switches()

    run = {"hip": (False, hip), "hip_staged": (True, hip), "torch_loop": (False, loop)}
    outs = {}
    for k, (lds, f) in run.items():  # warm every shape (code objects, allocator)
        set_lds(lds)
        for _ in range(3):
            outs[k] = f()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, (lds, f) in run.items():
            set_lds(lds)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.steps)
    set_lds(True)  # for the staging query below
    g = geom.cpu().numpy()
    cw, ch = g[:, 2] - g[:, 0] + 1, g[:, 3] - g[:, 1] + 1
    nv = int(valid.sum())
    staged = sum(ops.patch_staged(int(w), 3, torch.uint8, a.size) for w, v in zip(cw, valid.tolist()) if v)
    # what the extract launch has to move: every valid crop read once (uint8 × 3), every patch written
    bytes_in = int((cw * ch)[valid.cpu().numpy() != 0].sum()) * 3
    bytes_out = a.objects * 3 * a.size * a.size * 4
    del os.environ["SCFLOW_PATCH_LDS"]
    _lib.reload_switches()
    res = dict(frames=a.frames, height=a.height, width=a.width, objects=a.objects, size=a.size,
               rounds=a.rounds, steps=a.steps, valid=nv, staged=staged,
               crop_min=int(cw[valid.cpu().numpy() != 0].min()), crop_max=int(cw.max()),
               bytes_in=bytes_in, bytes_out=bytes_out,
               same_bits_staged_direct=bool(torch.equal(outs["hip"], outs["hip_staged"])),
               max_diff_vs_torch_levels=float((outs["hip"] - outs["torch_loop"]).abs().max() * 255))
    for k, v in times.items():
        res[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
        print(f"{k}: median {res[k]['median_ms']:.4f} ms/call (min {min(v):.4f}, max {max(v):.4f})")
    res["torch_over_hip"] = res["torch_loop"]["median_ms"] / res["hip"]["median_ms"]
    print(f"F={a.frames} frames of {a.height}×{a.width}, N={a.objects} objects ({nv} valid, crops "
          f"{res['crop_min']}-{res['crop_max']} px, {staged} of them staged under SCFLOW_PATCH_LDS=1), S={a.size}: "
          f"torch loop / HIP = {res['torch_over_hip']:.1f}×; the extract launch reads "
          f"{bytes_in / 1e6:.2f} MB and writes {bytes_out / 1e6:.2f} MB; staged and direct routes "
          f"{'equal' if res['same_bits_staged_direct'] else 'DIFFER'} bit for bit; max difference "
          f"from the torch loop {res['max_diff_vs_torch_levels']:.3f} levels")
    write_json(a, res)


def write_json(a, res):
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
