"""Per-launch times of the motion encoder's three 3×3 convs, the library's fp32 kernel against the
bf16 direct 3×3 kernel (``_lib.CONV_BF16_3X3``), measured the way DESIGN.md §24's GRU launches
were: each variant's launch bound once and issued ``--launches`` times back to back between two
device events, the variants alternating within a round, ``--rounds`` rounds, median [min, max] of
the per-launch time.  Every variant is listed twice (``rep`` 0 and 1: identical runs of the same
session, whose difference is the run-to-run spread the wiring rule of DESIGN.md §25 asks for).

usage: python tools/menc_launch_times.py [--rounds 9] [--launches 50] [--shapes 16x32x32,32x64x64]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, (c0, c1), cout, activation, output as channels [off, off + cout) of a buffer of `so` channels
CONVS = [("corr_net.1", (256, 0), 192, "ReLU", 0, 256),     # → MF[:, :192]
         ("flow_net.1", (128, 0), 64, "ReLU", 192, 256),    # → MF[:, 192:]
         ("out_net.0", (256, 0), 126, "ReLU", 256, 384)]    # → HX's motion channels, before the flow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--shapes", default="16x32x32,32x64x64")
    a = ap.parse_args()
    from scflow_amd import _lib, ops
    from scflow_amd.modules import ConvRunner
    names = {v: k for k, v in vars(_lib).items() if k.startswith("PLAN_")}
    for shape in a.shapes.split(","):
        n, h, w = (int(v) for v in shape.split("x"))
        M = n * h * w
        g = torch.Generator().manual_seed(0)
        variants = []
        for name, (c0, c1), cout, act, off, so in CONVS:
            src = torch.randn(M, c0 + c1, generator=g).cuda()
            out = torch.zeros(M, so, device="cuda")
            conv = torch.nn.Conv2d(c0 + c1, cout, 3, padding=1)
            with torch.no_grad():
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / np.sqrt(9 * (c0 + c1)))
            conv = conv.cuda()
            for fmt, label in ((None, "fp32"), (_lib.CONV_BF16_3X3, "bf16")):
                for rep in (0, 1):
                    r = ConvRunner([conv], act)
                    r.fmt = fmt
                    s0 = ops.Chan(src, 0, c0)
                    s1 = ops.Chan(src, c0, c1) if c1 else None
                    bl = r.bind(s0, ops.Chan(out, off, cout), n, h, w, src1=s1)
                    kind = names.get(ops.conv_plan_kind(bl.args), "?")
                    variants.append((f"{name} {label} rep={rep}", kind, r, bl, src, out, []))
        for _, _, _, bl, _, _, _ in variants:  # warm every variant (code objects, clocks)
            for _ in range(a.launches):
                bl()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.rounds):
            for v in variants:
                bl = v[3]
                bl()
                e0.record()
                for _ in range(a.launches):
                    bl()
                e1.record()
                e1.synchronize()
                v[6].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        print(f"n={n} h={h} w={w}  (us per launch: median [min, max] of {a.rounds} x {a.launches} "
              "back-to-back launches)", flush=True)
        for label, kind, *_, t in variants:
            print(f"  {label:26s} {kind:14s} {statistics.median(t):7.1f}  [{min(t):.1f}, {max(t):.1f}]",
                  flush=True)


if __name__ == "__main__":
    main()
