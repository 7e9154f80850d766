"""Timing of scene visibility against the composition it replaces, on the device,
alternating in one process.

usage: python tools/scene_bench.py [--frames 32] [--per-frame 8] [--lat 64] [--lon 128]
                                   [--rounds 7] [--steps 3] [--json out.json]

One shape: ``frames`` frames of 480×640 with ``per-frame`` instances each, ellipsoid meshes of
2·lon·(lat − 1) faces (64 × 128: 16 128), sensor depth given, stats and inst_id asked for.

* ``kernel``: ``scene.scene_visibility`` (one ``scflow_scene_visibility`` call, plus the wrapper's
  sort and un-permute).
* ``composition``: what a user could write without it — the existing ``Renderer`` at 640² (it is
  square), one image per instance, ``render_image=False``, eight frames' instances per call so that
  its [n, 640, 640] buffers fit; then torch for the distances, the visibility rule, the nearest
  visible instance, the three counts and the two boxes.  Its pixel convention is the renderer's
  (half a pixel off this call's), so the two sides' counts differ along silhouettes: the tool
  prints both totals and times the work, it does not compare values.

Every window lies between two device events around ``steps`` calls after a warm-up of both sides;
the median of ``rounds`` windows is reported.  No ratio is fixed in advance.
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

H, W, S = 480, 640, 640


def composition(renderer, labels, fidx, R, t, K, depth_test, delta, chunk_frames=8):
    """(stats [n, 11] int64 without the reserved column, inst_id [F, H, W]) from per-instance
    square renders and torch."""
    F = K.shape[0]
    n = labels.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H, device=R.device, dtype=torch.float32),
                            torch.arange(W, device=R.device, dtype=torch.float32), indexing="ij")
    stats = torch.empty(n, 11, dtype=torch.int64, device=R.device)
    inst = torch.empty(F, H, W, dtype=torch.int64, device=R.device)
    per = n // F
    big = torch.iinfo(torch.int64).max
    for f0 in range(0, F, chunk_frames):
        f1 = min(f0 + chunk_frames, F)
        sel = slice(f0 * per, f1 * per)
        fi = fidx[sel].long()
        z = renderer(R[sel], t[sel], K[fi], labels[sel].long())["fragments"].zbuf[:, :H, :W, 0]
        Kf = K[fi]
        ax = (xs[None] - Kf[:, 0, 2, None, None]) / Kf[:, 0, 0, None, None]
        ay = (ys[None] - Kf[:, 1, 2, None, None]) / Kf[:, 1, 1, None, None]
        s = torch.sqrt(ax * ax + ay * ay + 1.0)
        cov = z > 0
        M = torch.where(cov, z * s, torch.zeros(()).to(z))
        T = depth_test[fi] * s
        vis = cov & ((T == 0) | (M - T <= delta))
        valid = cov & (T > 0)
        m = len(fi)
        Mv = torch.where(vis, M, torch.full_like(M, float("inf"))).view(f1 - f0, per, H, W)
        best, arg = Mv.min(1)
        inst[f0:f1] = torch.where(torch.isfinite(best),
                                  arg + (torch.arange(f0, f1, device=R.device) * per)[:, None, None],
                                  torch.full_like(arg, -1))
        out = [cov.sum((1, 2)), valid.sum((1, 2)), vis.sum((1, 2))]
        for mask in (cov, vis):
            anyx, anyy = mask.any(1), mask.any(2)
            cols = torch.arange(W, device=R.device).expand(m, W)
            rows = torch.arange(H, device=R.device).expand(m, H)
            x0 = torch.where(anyx, cols, torch.full_like(cols, big)).min(1).values
            x1 = torch.where(anyx, cols, torch.full_like(cols, -1)).max(1).values
            y0 = torch.where(anyy, rows, torch.full_like(rows, big)).min(1).values
            y1 = torch.where(anyy, rows, torch.full_like(rows, -1)).max(1).values
            empty = x1 < 0
            neg = torch.full_like(x0, -1)
            out += [torch.where(empty, neg, x0), torch.where(empty, neg, y0),
                    torch.where(empty, neg, x1 - x0 + 1), torch.where(empty, neg, y1 - y0 + 1)]
        stats[sel] = torch.stack(out, 1)
    return stats, inst


def timed(fns, rounds, steps):
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / steps)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--per-frame", type=int, default=8)
    ap.add_argument("--lat", type=int, default=64)
    ap.add_argument("--lon", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_bench needs a GPU: a CPU run says nothing about these timings")
    from scflow_amd import scene, synthetic
    from scflow_amd.renderer import Renderer
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    C = 8
    meshes = {l: synthetic.ellipsoid_mesh(np.array([60.0 + 5 * l, 46.0 + 3 * l, 36.0 + 2 * l]), a.lat, a.lon)
              for l in range(C)}
    faces = len(meshes[0][1])
    rend = Renderer(image_size=(S, S), soft_blending=False, render_mask=False, render_image=False,
                    meshes=meshes).to(dev)
    table = scene.mesh_table(rend, dev)
    F, per = a.frames, a.per_frame
    n = F * per
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.linalg.det(q))[:, None, None]
    R = torch.from_numpy(q.astype(np.float32)).to(dev)
    t = torch.from_numpy(np.stack([rng.uniform(-220, 220, n), rng.uniform(-160, 160, n),
                                   rng.uniform(700, 1100, n)], 1).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rng.integers(0, C, n).astype(np.int32)).to(dev)
    fidx = torch.arange(F, dtype=torch.int32).repeat_interleave(per).to(dev)
    K = torch.tensor([[1066.778, 0, 312.9869], [0, 1067.487, 241.3109], [0, 0, 1]]).repeat(F, 1, 1).to(dev)
    dt = torch.full((F, H, W), 1000.0) + torch.from_numpy(rng.uniform(-150, 150, (F, H, W)).astype(np.float32))
    dt[torch.from_numpy(rng.random((F, H, W)) < 0.1)] = 0.0
    dt = dt.to(dev)

    ker = lambda: scene.scene_visibility(table, labels, fidx, R, t, K, H, W, dt, 15.0)  # noqa: E731
    ref = lambda: composition(rend, labels, fidx, R, t, K, dt, 15.0)  # noqa: E731
    ko, (cs, ci) = ker(), ref()
    ks = ko["stats"].long()
    res = dict(frames=F, per_frame=per, faces=faces, height=H, width=W, rounds=a.rounds, steps=a.steps,
               valid_pixels_kernel=int(ks[:, 1].sum()), valid_pixels_composition=int(cs[:, 1].sum()),
               visible_pixels_kernel=int(ks[:, 2].sum()), visible_pixels_composition=int(cs[:, 2].sum()),
               foreground_pixels_kernel=int((ko["inst_id"] >= 0).sum()),
               foreground_pixels_composition=int((ci >= 0).sum()))
    print(f"{n} instances of {faces} faces in {F} frames of {H}×{W}; silhouette pixels with a measurement "
          f"{res['valid_pixels_kernel']} (kernel) / {res['valid_pixels_composition']} (composition), "
          f"visible {res['visible_pixels_kernel']} / {res['visible_pixels_composition']}")
    tm = timed({"kernel": ker, "composition": ref}, a.rounds, a.steps)
    for k, v in tm.items():
        res[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
        print(f"{k}: median {res[k]['median_ms']:.3f} ms (min {min(v):.3f}, max {max(v):.3f})")
    res["composition_over_kernel"] = res["composition"]["median_ms"] / res["kernel"]["median_ms"]
    print(f"composition / kernel = {res['composition_over_kernel']:.2f}×")
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
