"""Standalone timing of the correlation branch's first two operators at the decoder's shapes:
the tiled lookup, corr_net.0 on the direct 1×1 kernel (bk 16) and on the wide 1×1 kernel
(SCFLOW_CONV_1X1W), and the two fused (scflow_corr_lookup_conv1x1).

    python tools/lookup_conv_bench.py [--batch 16 --size 32] [--reps 50] [--only fused] [--stamps]

--stamps: per-phase medians of one fused launch from the kernel's workgroup stamps.  The shipped
kernel has none; build a profiling variant and point SCFLOW_LIB at it:
    tools/build_variant.sh lc_stamps lookup_conv.hip -DLC_STAMPS
    SCFLOW_LIB=scflow_amd/lib/ab/lc_stamps.so python tools/lookup_conv_bench.py --only fused --stamps
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=32, help="feature map side")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="", help="substring of the case names to run")
    ap.add_argument("--stamps", action="store_true", help="phase stamps of one fused launch (LC_STAMPS build)")
    a = ap.parse_args()
    from scflow_amd import _lib, ops
    from scflow_amd.modules import ConvRunner
    n, h, w = a.batch, a.size, a.size
    M = n * h * w
    g = torch.Generator().manual_seed(0)
    f1 = torch.randn(n, 256, h, w, generator=g).cuda()
    f2 = torch.randn(n, 256, h, w, generator=g).cuda()
    pyr = ops.corr_pyramid_tiled(f1, f2, 4)
    flow = ((torch.rand(M, 2, generator=g) - 0.5) * 8).cuda()
    conv = torch.nn.Conv2d(324, 256, 1).cuda()
    r = ConvRunner([conv], "ReLU")
    corr = torch.empty(M, 324, device="cuda")
    out = torch.empty(M, 256, device="cuda")
    pk16, bias = r.packed(324, 0, w, 16)
    pkw, _ = r.packed(324, 0, w, _lib.CONV_1X1W)
    pk16 = pk16.clone()

    cases = {
        "lookup (tiled)": lambda: ops.corr_lookup(pyr, flow, n, h, w, 4, 4, out=ops.Chan.whole(corr),
                                                  flow_layout="nhwc", tiled=True),
        "corr_net.0 conv1x1_kernel": lambda: ops.conv2d(ops.Chan.whole(corr), pk16, bias, n, h, w, 256, 1,
                                                         1, 0, 0, "ReLU", out=ops.Chan.whole(out), bk=16),
        "corr_net.0 conv1x1w_kernel": lambda: ops.conv2d(ops.Chan.whole(corr), pkw, bias, n, h, w, 256, 1,
                                                          1, 0, 0, "ReLU", out=ops.Chan.whole(out),
                                                          bk=_lib.CONV_1X1W),
        "fused lookup+corr_net.0": lambda: ops.corr_lookup_conv1x1(pyr, flow, pkw, bias, ops.Chan.whole(out),
                                                                   n, h, w, 4, 4, 256),
    }
    for name, fn in cases.items():
        if a.only not in name:
            continue
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.reps
        fl = 2.0 * M * 324 * 256
        print(f"B={n} {h}x{w} {name:28s} {us:8.1f} us   {fl / us / 1e6:6.1f} TF(GEMM-equiv)", flush=True)
    if a.stamps:
        stamp_report(cases["fused lookup+corr_net.0"], -(-M // 64))


def stamp_report(run, nwg):
    """Per-phase medians over the workgroups of one fused launch (µs; stamps are 100 MHz ticks).
    Slots: 0 start; 1+l level l's regions in LDS, 5+l level l sampled (producers); 9+2(l-1),
    10+2(l-1) consumer phase l = 1..4 begins / ends; 17 epilogue stored."""
    import ctypes
    from scflow_amd import _lib
    lib = _lib.load()
    if not hasattr(lib, "scflow_debug_lookup_conv_stamps"):
        print("  (no stamps: this library was not built with -DLC_STAMPS)")
        return
    fn = lib.scflow_debug_lookup_conv_stamps
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p]
    nst = fn(None)
    st = torch.zeros(nwg * nst, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    fn(st.data_ptr())
    run()
    torch.cuda.synchronize()
    fn(None)
    v = st.view(nwg, nst).double().cpu() / 100.0
    t0 = v[:, 0].min().item()

    def med(i):
        return (v[:, i] - v[:, 0]).median().item()

    def dmed(i, j):
        return (v[:, i] - v[:, j]).median().item()

    print(f"  stamps: {nwg} WGs, starts spread {(v[:, 0].max().item() - t0):.2f} us, last epilogue at "
          f"{(v[:, 17].max().item() - t0):.2f} us, WG median {dmed(17, 0):.2f} us")
    print("  producers (us since WG start; region wait = loads returned and stored, sampling):")
    prev = 0
    for l in range(4):
        print(f"    level {l}: regions in LDS at {med(1 + l):6.2f} (+{dmed(1 + l, prev):5.2f})   "
              f"sampled at {med(5 + l):6.2f} (+{dmed(5 + l, 1 + l):5.2f})")
        prev = 5 + l
    print("  consumers (us since WG start; wait = phase start - previous phase end):")
    prev = 0
    for l in range(1, 5):
        b, e = 9 + 2 * (l - 1), 10 + 2 * (l - 1)
        print(f"    phase {l}: {med(b):6.2f} .. {med(e):6.2f}  (wait {dmed(b, prev):5.2f}, MFMA {dmed(e, b):5.2f})")
        prev = e
    print(f"    epilogue stored at {med(17):6.2f} (+{dmed(17, 16):5.2f})")


if __name__ == "__main__":
    main()
