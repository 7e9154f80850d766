"""Timing of the RAFT baseline decoders (RAFTDecoderMask, RAFTDecoder), interleaved in one process.

usage: python tools/raft_bench.py [--batch 16] [--size 256] [--iters 12] [--rounds 7] [--steps 10]
                                  [--json out.json] [--once KIND] [--train] [--pnp [--hyps 100]]

Each decoder is warmed up, then timed `rounds` times in round-robin order (`steps` forwards per
round, a device synchronise at both ends); prints the median, minimum and maximum ms per forward
of each and one JSON line with all of it.  It also prints the bytes the convex-upsampling launch
moves per call (from the shapes: logits + flow, Δflow, occlusion in; ×8 flow / occlusion and the
two next-flow destinations out), the figure a kernel trace's launch time is divided into.

`--train` times one eager training step of RAFTRefinerFlowMask instead (`train.step.TrainStep`:
forward, backward, gradient clipping at 1.0, AdamW; same defaults: B=16, 256², 12 iterations) and
prints the median ms per step over the rounds and one JSON line.

`--pnp` times `ops.pnp_ransac` alone (the batched RANSAC-PnP that turns the last ×8 flow into poses:
B=16, 256², `--hyps` 100 hypotheses) next to the RAFTDecoderMask forward it follows, alternating,
each window between two device events; prints both medians and one JSON line.

`--once KIND` runs `steps` forwards of one decoder (or `--once pnp_ransac`: `steps` PnP calls) and
nothing else: the run to put under `rocprofv3 --kernel-trace --stats` (a run of its own; end-to-end
numbers come from the untraced run).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("RAFTDecoderMask", "RAFTDecoder")


def decoder_cfg(kind, iters):
    """The decoder block of the reference's configs/refine_models/raft.py:40-48."""
    return dict(type=kind, net_type="Basic", num_levels=4, radius=4, iters=iters,
                corr_lookup_cfg=dict(align_corners=True), gru_type="SeqConv",
                act_cfg=dict(type="ReLU"))


def tail_bytes(batch, size, occlusion):
    """Bytes one scflow_convex_upsample launch has to move (fp32)."""
    m = batch * (size // 8) ** 2
    per_px = 576 + 2 + 2 + 64 * 2 + 2 + 2  # logits, lr, delta | ×8 flow, next0, next1
    if occlusion:
        per_px += 1 + 64
    return 4 * m * per_px


def refiner_cfg(iters):
    """The model block of the reference's configs/refine_models/raft.py (RAFTRefinerFlowMask)."""
    enc = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic")
    seq = dict(type="SequenceLoss", gamma=0.8)
    return dict(type="RAFTRefinerFlowMask", cxt_channels=128, h_channels=128, seperate_encoder=False,
                max_flow=400., filter_invalid_flow_by_mask=True, filter_invalid_flow_by_depth=False,
                encoder=dict(enc, norm_cfg=dict(type="IN")), cxt_encoder=dict(enc, norm_cfg=dict(type="BN")),
                decoder=decoder_cfg(KINDS[0], iters),
                flow_loss_cfg=dict(seq, loss_func_cfg=dict(type="RAFTLoss", loss_weight=1.0, max_flow=400.)),
                occlusion_loss_cfg=dict(seq, loss_func_cfg=dict(type="L1Loss", loss_weight=100.)))


def train(a):
    """One eager training step of RAFTRefinerFlowMask (forward, backward, clip at 1.0, AdamW) on a
    fixed synthetic batch: the median ms per step over `rounds` rounds of `steps` steps."""
    import numpy as np
    from scflow_amd import MODELS, synthetic
    from scflow_amd.train.step import TrainStep
    dev = torch.device("cuda")
    r = MODELS.build(refiner_cfg(a.iters))
    for i, m in enumerate((r.real_encoder, r.context, r.decoder)):
        synthetic.fill_module_(m, seed=(1, 2, 0)[i])
    with torch.no_grad():
        r.decoder.mask_pred.predict_layer.weight.mul_(32.0)
    r = r.to(dev)
    batch = {}
    for k, v in synthetic.make_train_batch(a.batch, a.size, seed=0).items():
        x = torch.from_numpy(np.ascontiguousarray(v))
        batch[k] = (x.float() if x.is_floating_point() else x).to(dev)
    step = TrainStep(r, None, None, max_norm=1.0)
    losses = [float(step(batch)["loss"]) for _ in range(3)]  # warm-up (packing, allocator)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = step(batch)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / a.steps * 1e3)
    res = dict(mode="train", kind="RAFTRefinerFlowMask", batch=a.batch, size=a.size, iters=a.iters,
               rounds=a.rounds, steps=a.steps, median_ms=statistics.median(times), min_ms=min(times),
               max_ms=max(times), warmup_losses=losses, last_loss=float(out["loss"]))
    print(f"RAFTRefinerFlowMask training step: median {res['median_ms']:.2f} ms/step "
          f"(min {min(times):.2f}, max {max(times):.2f}); B={a.batch}, {a.size}², {a.iters} iterations")
    return res


def pnp_inputs(a, dev):
    """flow, depth, R, t, K of a synthetic scene batch: the ground-truth flow of a known pose (the
    reference pose perturbed) with 30 % of the rendered pixels moved by 10-40 px, the pattern the
    RANSAC-PnP tests use."""
    import numpy as np
    from scflow_amd import ops, synthetic
    sc = synthetic.make_scene(a.batch, a.size, seed=0)
    tg = synthetic.make_train_targets(sc, a.size, seed=0)
    T = lambda k, d=sc: torch.from_numpy(np.ascontiguousarray(d[k])).to(dev)  # noqa: E731
    depth, K, R, t = T("depth"), T("internel_k"), T("ref_rotation"), T("ref_translation")
    flow = ops.pose_flow(T("gt_rotation", tg), T("gt_translation", tg), K,
                         ops.lift_points(depth, K, R, t), 0.0)
    g = torch.Generator(device=dev).manual_seed(0)
    moved = (torch.rand(depth.shape, device=dev, generator=g) < 0.3) & (depth > 0)
    mag = 10 + 30 * torch.rand(depth.shape, device=dev, generator=g)
    ang = 6.2831853 * torch.rand(depth.shape, device=dev, generator=g)
    flow = flow + moved[:, None] * torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], 1)
    return flow.contiguous(), depth, R, t, K


def pnp(a, dec, inp):
    """`ops.pnp_ransac` alone (lift → compact → hypotheses → score → refine) and the decoder forward
    it follows, alternating in one process, each timed with device events around `steps` calls."""
    from scflow_amd import ops
    dev = torch.device("cuda")
    args = pnp_inputs(a, dev)
    run = {"pnp_ransac": lambda: ops.pnp_ransac(*args, hyps=a.hyps), KINDS[0]: lambda: dec(**inp)}
    for f in run.values():  # warm every shape (code objects, packing, allocator)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, f in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                out = f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.steps)
    ok, inl = run["pnp_ransac"]()[2:]
    res = dict(mode="pnp", batch=a.batch, size=a.size, iters=a.iters, hyps=a.hyps, rounds=a.rounds,
               steps=a.steps, ok=int(ok.sum()), inliers=inl.tolist(),
               valid_pixels=(args[1] > 0).flatten(1).sum(1).tolist())
    for k, v in times.items():
        res[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
        print(f"{k}: median {res[k]['median_ms']:.3f} ms/call (min {min(v):.3f}, max {max(v):.3f}); "
              f"B={a.batch}, {a.size}²" + (f", {a.hyps} hypotheses" if k == "pnp_ransac"
                                           else f", {a.iters} iterations"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--pnp", action="store_true")
    ap.add_argument("--hyps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--once", default=None, choices=KINDS + ("pnp_ransac",))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("raft_bench.py needs a GPU (a CPU run measures nothing)")
    if a.once == "pnp_ransac":
        from scflow_amd import ops
        args = pnp_inputs(a, torch.device("cuda"))
        for _ in range(a.steps):
            ok = ops.pnp_ransac(*args, hyps=a.hyps)[2]
        torch.cuda.synchronize()
        print(f"pnp_ransac: {a.steps} calls, B={a.batch}, {a.size}², {a.hyps} hypotheses; "
              f"{int(ok.sum())} of {a.batch} poses found")
        return
    if a.train:
        line = json.dumps(train(a))
        print(line)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                f.write(line + "\n")
        return
    from scflow_amd import MODELS, synthetic
    dev = torch.device("cuda")
    raw = synthetic.make_decoder_inputs(a.batch, a.size, seed=0)
    h = a.size // 8
    inp = dict(feat1=torch.from_numpy(raw["feat_render"]).to(dev),
               feat2=torch.from_numpy(raw["feat_real"]).to(dev),
               flow=torch.zeros(a.batch, 2, h, h, device=dev),
               h_feat=torch.from_numpy(raw["h_feat"]).to(dev),
               cxt_feat=torch.from_numpy(raw["cxt_feat"]).to(dev))
    kinds = (a.once,) if a.once else (KINDS[:1] if a.pnp else KINDS)
    decs = {}
    for kind in kinds:
        dec = MODELS.build(decoder_cfg(kind, a.iters))
        synthetic.fill_module_(dec)
        with torch.no_grad():  # a softmax that is not flat (the golden fixtures' gain)
            dec.mask_pred.predict_layer.weight.mul_(32.0)
        decs[kind] = dec.to(dev).eval()
    if a.once:
        for _ in range(a.steps):
            decs[a.once](**inp)
        torch.cuda.synchronize()
        print(f"{a.once}: {a.steps} forwards of {a.iters} iterations, B={a.batch}, {a.size}²; "
              f"convex tail moves {tail_bytes(a.batch, a.size, a.once == KINDS[0])} B per launch")
        return
    if a.pnp:
        line = json.dumps(pnp(a, decs[KINDS[0]], inp))
        print(line)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                f.write(line + "\n")
        return
    for dec in decs.values():  # warm every shape (packing, allocator, code objects)
        for _ in range(3):
            dec(**inp)
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for kind in kinds:
            dec = decs[kind]
            dec(**inp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                dec(**inp)
            torch.cuda.synchronize()
            times[kind].append((time.perf_counter() - t0) / a.steps * 1e3)
    res = dict(batch=a.batch, size=a.size, iters=a.iters, rounds=a.rounds, steps=a.steps)
    for kind in kinds:
        v = times[kind]
        res[kind] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v),
                         ms_per_iteration=statistics.median(v) / a.iters, plan=decs[kind].last_plan,
                         tail_bytes=tail_bytes(a.batch, a.size, kind == KINDS[0]))
        print(f"{kind}: median {res[kind]['median_ms']:.3f} ms/forward "
              f"(min {min(v):.3f}, max {max(v):.3f}; {res[kind]['ms_per_iteration']:.3f} ms/iteration)")
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
