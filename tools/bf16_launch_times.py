"""Per-launch times of the convs that have an opt-in bf16 direct kernel, the library's fp32 kernel
against the bf16 one, by family:

  gru   the SepConvGRU's z|r and q launches, 1×5 and 5×1, context hoisted (256 → 256 / 128
        channels from c0 = c1 = 128: hidden state or r·h, and the motion features), F(4,5) fp32
        against ``_lib.CONV_BF16``
  menc  the motion encoder's three 3×3 convs, the library's fp32 kernel against
        ``_lib.CONV_BF16_3X3``
  enc   the RAFT encoders' stride-1 3×3 convs with their fused normalisation, fp32 against
        ``_lib.CONV_BF16_3X3N``: the per-launch part of tools/enc_bench.py

One method for all: each variant's launch is recorded once and issued ``--launches`` times back to
back between two device events, the variants alternating within a round, ``--rounds`` rounds,
median [min, max] of the per-launch time.  Every variant is listed twice (``rep`` 0 and 1:
identical runs of the same process, whose difference is the run-to-run spread the wiring rules of
DESIGN.md §25 / §26 ask for).  With more than one family each runs in a child process of its own
under ``--timeout`` seconds, and the first that fails ends the run.

usage: python tools/bf16_launch_times.py [--family gru,menc,enc] [--rounds 9] [--launches 50]
           [--shapes 16x32x32,32x64x64] [--sizes 256,512] [--batch512 16] [--timeout 300]
"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

# name, (c0, c1), cout, activation, output as channels [off, off + cout) of a buffer of `so` channels
MENC_CONVS = [("corr_net.1", (256, 0), 192, "ReLU", 0, 256),     # → MF[:, :192]
              ("flow_net.1", (128, 0), 64, "ReLU", 192, 256),    # → MF[:, 192:]
              ("out_net.0", (256, 0), 126, "ReLU", 256, 384)]    # → HX's motion channels, before the flow


def menc_variants(n, h, w):
    """[(label, plan kind, recorded launch, keep-alive, times)]: per conv, fp32 and bf16, each twice."""
    from scflow_amd import _lib, ops
    from scflow_amd.modules import ConvRunner
    M = n * h * w
    g = torch.Generator().manual_seed(0)
    variants = []
    for name, (c0, c1), cout, act, off, so in MENC_CONVS:
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
                kind, bl = record(r, s0, ops.Chan(out, off, cout), n, h, w, src1=s1)
                variants.append((f"{name} {label} rep={rep}", kind, bl, (r, src, out), []))
    return variants


def gru_variants(n, h, w):
    """The same list for the GRU's four launches as ``ConvGRU.step`` issues them with the
    context hoisted: z|r (epilogue writes z and r·h) and q (epilogue updates h), 1×5 then 5×1."""
    from scflow_amd import _lib, ops
    from scflow_amd.modules import ConvGRU, ConvRunner
    hc, cxt = 128, 128
    M = n * h * w
    g = torch.Generator().manual_seed(0)
    gru = ConvGRU(hc, cxt + hc, "SeqConv")
    with torch.no_grad():
        for p in gru.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / np.sqrt(5 * 3 * hc))
    gru = gru.cuda()
    hx = torch.randn(M, 3 * hc, generator=g).cuda()  # h | context | motion
    hx[:, :hc].tanh_()
    z, rh = torch.zeros(M, hc, device="cuda"), torch.zeros(M, hc, device="cuda")
    bmap = (torch.randn(M, 2 * 3 * hc, generator=g) * 0.1).cuda()
    hid, mot = ops.Chan(hx, 0, hc), ops.Chan(hx, hc + cxt, hc)
    variants = []
    keep = [(0, hc), (hc + cxt, 3 * hc)]  # the context's share arrives as the bias map
    for i, k in enumerate(("1x5", "5x1")):
        cz, cr, cq = gru.conv_z[i].conv, gru.conv_r[i].conv, gru.conv_q[i].conv
        for fmt, label in ((None, "f45_fp32"), (_lib.CONV_BF16, "bf16")):
            for rep in (0, 1):
                rzr = ConvRunner([cz, cr], "Sigmoid", in_select=keep, with_bias=False)
                rq = ConvRunner([cq], "Tanh", in_select=keep, with_bias=False)
                rzr.fmt = rq.fmt = fmt
                bzr = record(rzr, hid, None, n, h, w, src1=mot, epilogue=_lib.EPI_GRU_ZR, gate=ops.Chan.whole(z),
                             rh=ops.Chan.whole(rh), hid=hid, bias_map=ops.Chan(bmap, i * 3 * hc, 2 * hc))
                bq = record(rq, ops.Chan.whole(rh), None, n, h, w, src1=mot, epilogue=_lib.EPI_GRU_Q,
                            gate=ops.Chan.whole(z), hid=hid, bias_map=ops.Chan(bmap, i * 3 * hc + 2 * hc, hc))
                for name, (kind, bl) in (("zr", bzr), ("q ", bq)):
                    variants.append((f"{name} {k} {label} rep={rep}", kind, bl, (hx, z, rh, bmap), []))
    return variants


def record(r, *args, **kw):
    """(plan kind's name, the launch ``r.run(...)`` recorded for replay: ``ops.binding``)."""
    from scflow_amd import _lib, ops
    names = {v: k for k, v in vars(_lib).items() if k.startswith("PLAN_")}
    calls = []
    with ops.binding(calls, run=False):
        r.run(*args, **kw)
    return names.get(ops.conv_plan_kind(r.args(*args, **kw)), "?"), calls[0]


def by_shape(a, make):
    import enc_bench
    for shape in a.shapes.split(","):
        n, h, w = (int(v) for v in shape.split("x"))
        variants = make(n, h, w)
        enc_bench.time_variants(variants, a.rounds, a.launches, lambda v: v[2]())
        print(f"n={n} h={h} w={w}  (us per launch: median [min, max] of {a.rounds} x {a.launches} "
              "back-to-back launches)", flush=True)
        for label, kind, *_, t in variants:
            t = [1e3 * v for v in t]
            print(f"  {label:26s} {kind:14s} {statistics.median(t):7.1f}  [{min(t):.1f}, {max(t):.1f}]",
                  flush=True)
        del variants
        torch.cuda.empty_cache()


def enc(a):
    import enc_bench
    enc_bench.per_launch(a)


FAMILIES = {"gru": lambda a: by_shape(a, gru_variants), "menc": lambda a: by_shape(a, menc_variants),
            "enc": enc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", default="menc", help="comma-separated: " + ", ".join(FAMILIES))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--shapes", default="16x32x32,32x64x64", help="gru, menc: n x h x w of the feature maps")
    ap.add_argument("--sizes", default="256,512", help="enc: image sizes")
    ap.add_argument("--batch512", type=int, default=16, help="enc: images of 512² through the IN encoder")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per family's child process")
    a = ap.parse_args()
    families = a.family.split(",")
    unknown = [f for f in families if f not in FAMILIES]
    if unknown:
        ap.error(f"unknown family {unknown}; one of {sorted(FAMILIES)}")
    if len(families) > 1:  # a process per family, each under its own time limit; stop at the first failure
        for f in families:
            argv = [sys.executable, os.path.abspath(__file__), "--family", f] + [
                f"--{k}={getattr(a, k)}" for k in ("rounds", "launches", "shapes", "sizes", "batch512")]
            print(f"== family {f}", flush=True)
            status = subprocess.run(argv, timeout=a.timeout).returncode
            if status:
                sys.exit(f"family {f} ended with status {status}: stopping")
        return
    with torch.no_grad():
        FAMILIES[families[0]](a)


if __name__ == "__main__":
    main()
