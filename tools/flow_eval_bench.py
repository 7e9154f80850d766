"""Timing of flow validation against the composition it replaces, on the device,
alternating in one process.

usage: python tools/flow_eval_bench.py [--batch 32] [--size 256] [--rounds 9] [--steps 200]
                                       [--json out.json]

One shape: ``batch`` samples of ``size``² (``synthetic.make_train_batch``), a prediction and an
occlusion map on the device.  Both sides compute the reference's ``eval_epe_and_occ`` with
``reduction='total_mean'`` (nine 0-dim device tensors, no host synchronisation inside the window).

* ``fused``: ``flow_eval.eval_epe_and_occ`` — one ``scflow_flow_gt`` launch (GT flow + mask filter)
  and two ``scflow_flow_epe`` calls (two launches each).
* ``composition``: what a user writes today — ``ops.lift_points``, ``ops.pose_flow``,
  ``train.losses.filter_flow_by_mask`` (``grid_sample`` + ``where``) and ``cal_epe`` in torch, twice,
  plus the occlusion term.

Every variant is timed twice (``*_1``, ``*_2``), interleaved, so the spread of identical runs
stands beside the difference between the variants.  A window lies between two device events
around ``steps`` calls after a warm-up; the median of ``rounds`` windows is reported.  The tool
also prints the largest difference between the two sides' values.  No ratio is fixed in advance.
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


def torch_cal_epe(tgt, pred, max_flow, threshs=(1, 3, 5)):
    """cal_epe(reduction='total_mean'), models/utils/flow.py:64-88, in torch."""
    valid = torch.sum(tgt ** 2, dim=1).sqrt() < max_flow
    err = torch.sum((tgt - pred) ** 2, dim=1).sqrt()
    total = valid.sum() + 1e-10
    out = {"mean": (err * valid.to(err.dtype)).sum() / total}
    for t in threshs:
        out[f"{t}px"] = ((err < t) & valid).sum() / total
    return out


def composition(b, pred, occ, max_flow):
    from scflow_amd import ops
    from scflow_amd.train import losses
    pts = ops.lift_points(b["depth"], b["internel_k"], b["ref_rotation"], b["ref_translation"])
    flow = ops.pose_flow(b["gt_rotation"], b["gt_translation"], b["internel_k"], pts, max_flow)
    out = {f"epe_{k}": v for k, v in torch_cal_epe(flow, pred, max_flow).items()}
    noc = losses.filter_flow_by_mask(flow, b["gt_masks"], max_flow)
    out.update({f"epe_noc_{k}": v for k, v in torch_cal_epe(noc, pred, max_flow).items()})
    occ_gt = torch.sum(noc ** 2, dim=1).sqrt() < max_flow
    out["occ"] = torch.abs(occ_gt.to(occ.dtype) - occ).mean()
    return out


def timed(fns, rounds, steps):
    for f in fns.values():
        for _ in range(5):
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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_eval_bench needs a GPU: a CPU run says nothing about these timings")
    from scflow_amd import flow_eval, synthetic
    dev = torch.device("cuda")
    b = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
         for k, v in synthetic.make_train_batch(a.batch, a.size, seed=3).items()}
    rng = np.random.default_rng(0)
    max_flow = 400.0
    gt, _ = flow_eval.gt_flow(b["depth"], b["internel_k"], b["ref_rotation"], b["ref_translation"],
                              b["gt_rotation"], b["gt_translation"], max_flow)
    noise = torch.from_numpy(rng.normal(0, 2.5, tuple(gt.shape)).astype(np.float32)).to(dev)
    pred = torch.where(gt.abs() < 100, gt + noise, noise).contiguous()
    occ = torch.from_numpy(rng.uniform(0, 1, (a.batch, a.size, a.size)).astype(np.float32)).to(dev)

    fused = lambda: flow_eval.eval_epe_and_occ(  # noqa: E731
        pred, occ, b["depth"], b["gt_rotation"], b["gt_translation"], b["internel_k"],
        b["ref_rotation"], b["ref_translation"], b["gt_masks"], max_flow, "total_mean")
    comp = lambda: composition(b, pred, occ, max_flow)  # noqa: E731
    fo, co = fused(), comp()
    diff = {k: abs(float(fo[k]) - float(co[k])) for k in fo}
    hw = a.size * a.size
    # bytes the fused path moves: flow_gt reads depth + mask (1 B) and writes two flows; each
    # flow_epe reads two flows (the second also the occlusion)
    nbytes = a.batch * hw * ((4 + 1 + 16) + 16 + (16 + 4))
    res = dict(batch=a.batch, size=a.size, rounds=a.rounds, steps=a.steps, fused_bytes=nbytes,
               values={k: float(v) for k, v in fo.items()}, largest_value_difference=max(diff.values()))
    print(f"B = {a.batch}, {a.size}²: fused path moves {nbytes / 1e6:.1f} MB; values "
          + ", ".join(f"{k} {float(v):.6g}" for k, v in fo.items()))
    print(f"largest |fused − composition| over the nine values: {res['largest_value_difference']:.3e}")
    tm = timed({"fused_1": fused, "composition_1": comp, "fused_2": fused, "composition_2": comp},
               a.rounds, a.steps)
    for k, v in tm.items():
        res[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
        print(f"{k}: median {res[k]['median_ms'] * 1e3:.1f} µs (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})")
    f = statistics.median(tm["fused_1"] + tm["fused_2"])
    c = statistics.median(tm["composition_1"] + tm["composition_2"])
    res["composition_over_fused"] = c / f
    res["fused_gbytes_per_s"] = nbytes / (f * 1e-3) / 1e9
    print(f"composition / fused = {c / f:.2f}×; fused: {res['fused_gbytes_per_s']:.0f} GB/s of the bytes it needs")
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
