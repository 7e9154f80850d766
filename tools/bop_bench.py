"""Timing of the BOP pose-error kernels against the torch compositions a user could
write without them, on the device, alternating in one process.

usage: python tools/bop_bench.py [--n 256] [--points 8192] [--pairs 64] [--rounds 9] [--steps 20]
                                 [--json out.json]

* ``mssd_mspd``: N estimates of one class with P vertices and S ∈ {1, 315} symmetry transforms
  (``bop_metrics.mssd_mspd``, one launch) against a torch composition chunked over the symmetries
  so that its [N, chunk, P, 3] intermediates fit in memory.
* ``vsd_counts``: ``pairs`` (estimate, GT) pairs at 480×640, two objects per frame, ten tolerances,
  against its torch composition (a dozen elementwise passes and a reduction).

Every window lies between two device events around ``steps`` calls, after a warm-up of every
configuration; the median of ``rounds`` windows is reported with the algorithmic operations and
bytes of the shapes (what the definition needs, whatever the kernel does) and the rates they give.
No ratio is fixed in advance: the tool reports what it measures, also where a kernel loses.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SYM_CHUNK = 8  # symmetries per pass of the torch composition: [256, 8, 8192, 3] fp32 = 201 MB


def torch_mssd_mspd(pts, sym, Re, te, Rg, tg, K):
    """min over symmetries of max over vertices, SYM_CHUNK symmetries at a time."""
    pe = torch.einsum("nij,pj->npi", Re, pts) + te[:, None]                   # [N, P, 3]
    he = torch.einsum("nij,npj->npi", K, pe)
    ue = he[..., :2] / he[..., 2:]
    s_best = torch.full((Re.shape[0],), float("inf"), device=pts.device)
    p_best = s_best.clone()
    for c0 in range(0, sym.shape[0], SYM_CHUNK):
        T = sym[c0:c0 + SYM_CHUNK].view(-1, 3, 4)
        x = torch.einsum("sij,pj->spi", T[:, :, :3], pts) + T[:, None, :, 3]  # [s, P, 3]
        q = torch.einsum("nij,spj->nspi", Rg, x) + tg[:, None, None]          # [N, s, P, 3]
        s_best = torch.minimum(s_best, (pe[:, None] - q).norm(dim=-1).amax(-1).amin(-1))
        h = torch.einsum("nij,nspj->nspi", K, q)
        u = h[..., :2] / h[..., 2:]
        p_best = torch.minimum(p_best, (ue[:, None] - u).norm(dim=-1).amax(-1).amin(-1))
    return s_best, p_best


def torch_vsd_counts(de, dg, dt, fi, K, diam, taus, delta):
    n, h, w = de.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=de.device, dtype=torch.float32),
                            torch.arange(w, device=de.device, dtype=torch.float32), indexing="ij")
    ax = (xs[None] - K[:, 0, 2, None, None]) / K[:, 0, 0, None, None]
    ay = (ys[None] - K[:, 1, 2, None, None]) / K[:, 1, 1, None, None]
    s = torch.sqrt(ax * ax + ay * ay + 1.0)
    me, mg, mt = de * s, dg * s, dt[fi.long()] * s
    unseen = mt == 0
    vg = ((mg - mt <= delta) | unseen) & (mg > 0)
    ve = (((me - mt <= delta) | unseen) & (me > 0)) | (vg & (me > 0))
    inter = vg & ve
    r = (mg - me).abs() / diam[:, None, None]
    cost = (inter[..., None] & (r[..., None] >= taus)).sum((1, 2))
    return torch.cat([(vg | ve).sum((1, 2))[:, None], inter.sum((1, 2))[:, None], cost], 1).int()


def timed(fns, rounds, steps):
    """{name: [ms per call] per round}: the configurations alternate inside every round."""
    for f in fns.values():
        for _ in range(3):
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
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--torch-steps", type=int, default=2, help="calls per window of the S = 315 torch composition")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bop_bench needs a GPU: a CPU run says nothing about these timings")
    from scflow_amd import bop_metrics as bm
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    res = dict(n=a.n, points=a.points, pairs=a.pairs, rounds=a.rounds, steps=a.steps)

    def stats(name, v, flops, nbytes):
        med = statistics.median(v)
        res[name] = dict(median_ms=med, min_ms=min(v), max_ms=max(v), flops=flops, bytes=nbytes,
                         tflops=flops / med / 1e9, gbytes_per_s=nbytes / med / 1e6)
        print(f"{name}: median {med:.4f} ms (min {min(v):.4f}, max {max(v):.4f}); algorithmic "
              f"{flops / 1e9:.3f} GFLOP → {flops / med / 1e9:.2f} TFLOP/s, {nbytes / 1e6:.2f} MB → "
              f"{nbytes / med / 1e6:.1f} GB/s")

    # ---- MSSD / MSPD: one class, P vertices, S symmetries
    n, P = a.n, a.points
    pts = (torch.rand(P, 3, generator=g) * 160 - 80).to(dev)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))
    Rg = (q * torch.linalg.det(q)[:, None, None]).to(dev)
    w = torch.randn(n, 3, generator=g) * 0.1
    wx = torch.zeros(n, 3, 3)
    wx[:, 0, 1], wx[:, 0, 2], wx[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
    Re = Rg @ torch.linalg.matrix_exp(wx - wx.transpose(1, 2)).to(dev)
    tg = torch.cat([torch.rand(n, 2, generator=g) * 300 - 150, torch.rand(n, 1, generator=g) * 1000 + 500], 1).to(dev)
    te = tg + (torch.rand(n, 3, generator=g) * 40 - 20).to(dev)
    K = torch.tensor([[1066.778, 0, 312.9869], [0, 1067.487, 241.3109], [0, 0, 1]]).repeat(n, 1, 1).to(dev)
    labels = torch.zeros(n, dtype=torch.int32, device=dev)
    counts = torch.tensor([P], dtype=torch.int32, device=dev)
    for S, info in ((1, {}), (315, {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})):
        sym, off = bm.symmetry_table({"1": info}, 1, dev)
        assert sym.shape[0] == S
        ker = lambda: bm.mssd_mspd(pts[None], counts, sym, off, labels, Re, te, Rg, tg, K)  # noqa: E731
        ref = lambda: torch_mssd_mspd(pts, sym, Re, te, Rg, tg, K)  # noqa: E731
        (ks, kp), (ts, tp) = ker(), ref()
        print(f"S={S}: max |kernel − torch| MSSD {float((ks - ts).abs().max()):.3e}, MSPD "
              f"{float((kp - tp).abs().max()):.3e} px")
        t = timed({"kernel": ker}, a.rounds, a.steps)
        t.update(timed({"torch": ref}, a.rounds, a.steps if S == 1 else a.torch_steps))
        # per (estimate, symmetry, vertex): R̄S·x + t 18, difference and norm² 8, K·X 18, the division,
        # difference and norm² 7; per (estimate, vertex): R̂x + t̂ and its projection 38
        flops = n * P * (S * 51 + 38)
        nbytes = n * P * 12 + S * 48 + n * 33 * 4 + n * 8
        stats(f"mssd_mspd_S{S}_kernel", t["kernel"], flops, nbytes)
        stats(f"mssd_mspd_S{S}_torch", t["torch"], flops, nbytes)
        res[f"mssd_mspd_S{S}_torch_over_kernel"] = res[f"mssd_mspd_S{S}_torch"]["median_ms"] / \
            res[f"mssd_mspd_S{S}_kernel"]["median_ms"]

    # ---- VSD counts: 480×640, two objects per frame
    m, h, wd = a.pairs, 480, 640
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(wd, dtype=torch.float32), indexing="ij")
    cx, cy = torch.rand(m, generator=g) * 400 + 120, torch.rand(m, generator=g) * 280 + 100
    base = torch.rand(m, generator=g) * 200 + 700
    blob = ((xs[None] - cx[:, None, None]) ** 2 + (ys[None] - cy[:, None, None]) ** 2) <= 90.0 ** 2
    dg = torch.where(blob, base[:, None, None] + 0.5 * (xs[None] - cx[:, None, None]), torch.zeros(()))
    de = torch.roll(dg, (2, -3), (1, 2)) + torch.where(dg > 0, torch.rand(m, 1, 1, generator=g) * 80 - 40, torch.zeros(()))
    de = torch.where(torch.roll(dg, (2, -3), (1, 2)) > 0, de, torch.zeros(()))
    fi = (torch.arange(m) // 2).int()
    dt = torch.full((int(fi.max()) + 1, h, wd), 800.0) + torch.rand(int(fi.max()) + 1, h, wd, generator=g) * 120 - 60
    dt[torch.rand(dt.shape, generator=g) < 0.15] = 0.0
    de, dg, dt, fi = de.to(dev), dg.to(dev), dt.to(dev), fi.to(dev)
    Kv = K[:1].repeat(m, 1, 1)
    diam = (torch.rand(m, generator=g) * 100 + 100).to(dev)
    taus = torch.tensor(bm.BOP19_TAUS, device=dev)
    ker = lambda: bm.vsd_counts(de, dg, dt, fi, Kv, diam, taus, 15.0)  # noqa: E731
    ref = lambda: torch_vsd_counts(de, dg, dt, fi, Kv, diam, taus, 15.0)  # noqa: E731
    dk = (ker().long() - ref().long()).abs()
    print(f"vsd_counts: union {int(ker()[:, 0].sum())} pixels, max |kernel − torch| count {int(dk.max())}")
    t = timed({"kernel": ker, "torch": ref}, a.rounds, a.steps)
    # per pixel and pair: the distance factor ~12, three distances 3, visibility ~10, the cost ~4 + n_taus
    flops = m * h * wd * (29 + len(bm.BOP19_TAUS))
    nbytes = (2 * m + dt.shape[0]) * h * wd * 4
    stats("vsd_counts_kernel", t["kernel"], flops, nbytes)
    stats("vsd_counts_torch", t["torch"], flops, nbytes)
    res["vsd_counts_torch_over_kernel"] = res["vsd_counts_torch"]["median_ms"] / res["vsd_counts_kernel"]["median_ms"]
    for k in ("mssd_mspd_S1", "mssd_mspd_S315", "vsd_counts"):
        print(f"{k}: torch / kernel = {res[k + '_torch_over_kernel']:.2f}×")
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
