"""The RAFT encoders' stride-1 3×3 convs: the fp32 launch the encoder issues today (F(2×2,3×3) at
widths 32 / 64 / 128, the encoder's direct MFMA conv at 256) against the bf16 direct conv
(``_lib.CONV_BF16_3X3N``), and the whole ``extract_feat`` / ``get_pose`` with ``enc_bf16`` off / on.

Per launch (tools/bf16_launch_times.py's method; its ``--family enc`` runs this part): per stage (res_layer1 / 2 / 3) and form — "IN":
the producer's InstanceNorm + ReLU fused on load, the shared feature encoder's conv2; "BN": the
eval-BatchNorm affine + residual + ReLU epilogue, the context encoder's conv2 — each variant's
launch is bound once and issued ``--launches`` times back to back between two device events, the
variants alternating within a round, ``--rounds`` rounds, median [min, max] of the per-launch
time.  Every variant is listed twice (``rep`` 0 and 1: identical runs, whose difference is the
run-to-run spread DESIGN.md §26's wiring rule asks for).  Shapes: BASELINE configs[2]'s — 64
images of 256² through the shared encoder (IN), 32 through the context encoder (BN) — and 512²
images at ``--batch512`` / half of it.

End to end (``--e2e``): ``extract_feat`` and ``get_pose`` at configs[2] (B = 32, 256², 8
iterations) with the knob off / on and with all three bf16 knobs, every variant twice,
alternating, ``--rounds`` rounds of ``--steps`` calls.

usage: python tools/enc_bench.py [--rounds 9] [--launches 30] [--sizes 256,512] [--batch512 16] [--e2e]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = [("res_layer1", 64, 2), ("res_layer2", 96, 4), ("res_layer3", 128, 8)]  # name, channels, image / map


def launch_variants(n_in, n_bn, size):
    """[(label, kernel, calls, keep-alive)] for one image size: per stage and form, fp32 and bf16,
    each twice."""
    from scflow_amd import _lib, encoder, ops
    g = torch.Generator().manual_seed(0)
    out = []
    for stage, c, div in STAGES:
        s = size // div
        conv = torch.nn.Conv2d(c, c, 3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / np.sqrt(9 * c))
        conv = conv.cuda()
        for form, n in (("IN", n_in), ("BN", n_bn)):
            x = torch.randn(n, s, s, c, generator=g).cuda()
            y = torch.empty_like(x)
            if form == "IN":
                fused = dict(in_scale=(torch.rand(n, c, generator=g) + 0.5).cuda(),
                             in_shift=(torch.randn(n, c, generator=g) * 0.2).cuda())
            else:
                fused = dict(out_scale=(torch.rand(c, generator=g) + 0.5).cuda(),
                             out_shift=(torch.randn(c, generator=g) * 0.2).cuda(),
                             res=torch.randn(n, s, s, c, generator=g).cuda(), act="ReLU")
            for label in ("fp32", "bf16"):
                for rep in (0, 1):
                    calls = []
                    with ops.binding(calls):
                        if label == "bf16":
                            encoder._conv3x3(_lib.CONV_BF16_3X3N, conv, x, y, n, s, s, c, **fused)
                            kernel = "conv3_bf16"
                        elif encoder._wino_ok(conv, s, s, c):
                            encoder._conv3x3(_lib.CONV_WINO, conv, x, y, n, s, s, c, **fused)
                            kernel = "F(2x2,3x3)"
                        else:
                            ops.enc_conv(x, encoder._packed(conv), encoder._bias(conv), n, s, s, c, c, 3,
                                         1, 1, y, **fused)
                            kernel = "enc_conv"
                    out.append((f"{stage} {form} n={n} {s}x{s}x{c} {label} rep={rep}", kernel, calls,
                                (x, y, fused, conv), []))
    return out


def time_variants(variants, rounds, reps, run):
    for v in variants:  # warm every variant (code objects, clocks)
        for _ in range(reps):
            run(v)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for v in variants:
            run(v)
            e0.record()
            for _ in range(reps):
                run(v)
            e1.record()
            e1.synchronize()
            v[-1].append(e0.elapsed_time(e1) / reps)


def per_launch(a):
    for size in (int(v) for v in a.sizes.split(",")):
        n_in = 64 if size == 256 else a.batch512
        n_bn = n_in // 2
        variants = launch_variants(n_in, n_bn, size)

        def run(v):
            for c in v[2]:
                c()
        time_variants(variants, a.rounds, a.launches, run)
        print(f"{size}x{size} images, {n_in} through the IN encoder, {n_bn} through the BN encoder  "
              f"(us per launch: median [min, max] of {a.rounds} x {a.launches} back-to-back launches)",
              flush=True)
        for label, kernel, *_, t in variants:
            t = [1e3 * v for v in t]
            print(f"  {label:48s} {kernel:11s} {statistics.median(t):8.1f}  [{min(t):.1f}, {max(t):.1f}]",
                  flush=True)
        del variants
        torch.cuda.empty_cache()


def end_to_end(a):
    import bench
    dev = torch.device("cuda")
    r = bench.build_refiner(8, dev)
    rin = bench.make_refine_inputs(32, 256, seed=1000, device=dev)
    knobs = [("off", (False, False, False)), ("enc_bf16", (True, False, False)),
             ("gru+menc", (False, True, True)), ("all three", (True, True, True))]
    fns = [("extract_feat", lambda: r.extract_feat(rin["render_images"], rin["real_images"])),
           ("get_pose", lambda: r.get_pose(**rin))]
    for fname, fn in fns:
        variants = [(f"{fname} {k} rep={rep}", flags, []) for k, flags in knobs for rep in (0, 1)
                    if fname == "get_pose" or k in ("off", "enc_bf16")]

        def run(v):
            r.enc_bf16, r.decoder.gru_bf16, r.decoder.menc_bf16 = v[1]
            with torch.no_grad():
                fn()
        time_variants(variants, a.rounds, a.steps, run)
        r.enc_bf16 = r.decoder.gru_bf16 = r.decoder.menc_bf16 = False
        print(f"{fname}, B=32, 256x256, 8 iterations  (ms per call: median [min, max] of {a.rounds} x "
              f"{a.steps} calls)", flush=True)
        for label, _, t in variants:
            print(f"  {label:32s} {statistics.median(t):8.3f}  [{min(t):.3f}, {max(t):.3f}]", flush=True)
    r.enc_bf16 = True
    r.extract_feat(rin["render_images"][:1], rin["real_images"][:1])
    r.enc_bf16 = False
    print("convs on bf16 with enc_bf16:", ", ".join(r.real_encoder.last_bf16) or "none", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--batch512", type=int, default=16)
    ap.add_argument("--e2e", action="store_true", help="the end-to-end part instead of the per-launch table")
    a = ap.parse_args()
    from scflow_amd import encoder
    print("BF16_STAGES =", encoder.BF16_STAGES, flush=True)
    with torch.no_grad():
        end_to_end(a) if a.e2e else per_launch(a)


if __name__ == "__main__":
    main()
