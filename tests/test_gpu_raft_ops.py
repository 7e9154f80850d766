"""GPU: scflow_convex_upsample (RAFT's convex ×8 upsampling of the flow and the occlusion, one
launch) against a float64 torch restatement (``unfold`` + ``softmax``,
tests/raft_restatement.py).

Bound: the kernel's maximum absolute error is at most 4 × the error of the SAME composition run in
float32 torch on the same inputs, computed here at run time (the factor allows for the hardware
exp2 the kernel uses).  The next-flow destinations must equal ``lr + delta`` bit for bit, and
nothing outside the outputs may be written (sentinel bands around every output).
"""
import numpy as np
import pytest
import torch

from tests import raft_restatement as rr

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1, 1, 1),    # every neighbour padded
              (2, 2, 3),
              (2, 5, 7),    # odd sizes, all four borders, a partial strip
              (1, 32, 32)]  # several full strips per row, many workgroups
# (delta given, occ given, logit pixel stride)
VARIANTS = [(True, True, 576), (False, True, 580), (True, False, 580), (False, False, 576)]
PAD = 32  # floats of sentinel before and after each output (keeps 16-byte alignment)


def _guarded(shape, dev="cuda"):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), float("nan"), device=dev)
    return buf, buf[PAD:PAD + n].view(*shape)


def _untouched(buf):
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all())


def _case(n, h, w, with_delta, with_occ, ls, seed, logit_std=8.0):
    g = torch.Generator().manual_seed(seed)
    m = n * h * w
    return dict(logits=torch.randn(m, ls, generator=g) * logit_std,
                lr=(torch.rand(m, 2, generator=g) - 0.5) * 6,
                delta=torch.randn(m, 2, generator=g) * 0.5 if with_delta else None,
                occ=torch.rand(m, 1, generator=g) if with_occ else None)


def _restate(c, n, h, w, dtype):
    """The composition in ``dtype`` on the kernel's own inputs (x = lr + delta as float32 holds it)."""
    x = c["lr"] if c["delta"] is None else c["lr"] + c["delta"]
    nchw = lambda a: a.view(n, h, w, -1).permute(0, 3, 1, 2).contiguous().to(dtype)  # noqa: E731
    lg = nchw(c["logits"][:, :576])
    flow = rr.convex_upsample(nchw(x), lg, 0.25, 8.0)
    occ = None if c["occ"] is None else rr.convex_upsample(nchw(c["occ"]), lg, 0.25, 1.0)
    return x, flow, occ


def _run_kernel(c, n, h, w, ls, next_stride=384, next_off=382):
    from scflow_amd import ops
    from scflow_amd.ops import Chan
    dev = "cuda"
    lg = c["logits"].to(dev)
    m = n * h * w
    fb, flow_up = _guarded((n, 2, 8 * h, 8 * w))
    ob, occ_up = _guarded((n, 1, 8 * h, 8 * w))
    n0b, next0 = _guarded((m, 2))
    n1b, next1 = _guarded((m, next_stride))
    ops.convex_upsample(Chan(lg, 0, 576), c["lr"].to(dev),
                        None if c["delta"] is None else c["delta"].to(dev),
                        None if c["occ"] is None else c["occ"].to(dev), n, h, w, flow_up,
                        None if c["occ"] is None else occ_up, next0=Chan.whole(next0),
                        next1=Chan(next1, next_off, 2))
    torch.cuda.synchronize()
    for nm, b in (("flow_up", fb), ("occ_up", ob), ("next0", n0b), ("next1", n1b)):
        assert _untouched(b), f"{nm}: written outside the output"
    if c["occ"] is None:
        assert bool(torch.isnan(ob).all()), "occ_up written without occ"
    assert bool(torch.isnan(next1[:, :next_off]).all()), "next1: written outside its two channels"
    return flow_up.cpu(), occ_up.cpu(), next0.cpu(), next1[:, next_off:next_off + 2].cpu()


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"delta{int(v[0])}-occ{int(v[1])}-ls{v[2]}")
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "n%d-%dx%d" % g)
def test_convex_upsample_matches_float64_restatement(geom, variant):
    n, h, w = geom
    with_delta, with_occ, ls = variant
    c = _case(n, h, w, with_delta, with_occ, ls, seed=100 * h + w + 7 * ls)
    x, ref_flow, ref_occ = _restate(c, n, h, w, torch.float64)
    _, f32_flow, f32_occ = _restate(c, n, h, w, torch.float32)
    flow_up, occ_up, next0, next1 = _run_kernel(c, n, h, w, ls)
    # the next iteration's flow, both destinations: lr + delta bit for bit
    assert torch.equal(next0, x) and torch.equal(next1, x)
    err = float((flow_up.double() - ref_flow).abs().max())
    bound = 4 * float((f32_flow.double() - ref_flow).abs().max())
    print(f"flow: kernel max err {err:.3e}, float32 torch {bound / 4:.3e} (bound {bound:.3e})")
    assert err <= bound
    if with_occ:
        err = float((occ_up.double() - ref_occ).abs().max())
        bound = 4 * float((f32_occ.double() - ref_occ).abs().max())
        print(f"occ:  kernel max err {err:.3e}, float32 torch {bound / 4:.3e} (bound {bound:.3e})")
        assert err <= bound


def test_convex_upsample_large_logits_stay_finite_and_convex():
    """Raw logits of magnitude 400: 0.25 · 400 = 100 overflows exp without the maximum subtracted.
    The outputs are finite convex combinations: inside the (zero-padded) neighbourhood's min / max
    up to the combination's rounding — nine fused multiply-adds, one division and one scaling, each
    at most half an ulp of a value bounded by value_scale · max|v|: 16 · 2^-24 · that bound."""
    n, h, w = 2, 5, 7
    c = _case(n, h, w, True, True, 576, seed=9)
    g = torch.Generator().manual_seed(10)
    sign = torch.where(torch.rand(c["logits"].shape, generator=g) < 0.5, -1.0, 1.0)
    c["logits"] = 400.0 * sign + torch.randn(c["logits"].shape, generator=g)
    x, ref_flow, ref_occ = _restate(c, n, h, w, torch.float64)
    flow_up, occ_up, _, _ = _run_kernel(c, n, h, w, 576)
    assert bool(torch.isfinite(flow_up).all()) and bool(torch.isfinite(occ_up).all())
    nchw = lambda a: a.view(n, h, w, -1).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    for up, v, vs in ((flow_up, nchw(x), 8.0), (occ_up, nchw(c["occ"]), 1.0)):
        ch = v.shape[1]
        nb = torch.nn.functional.unfold(vs * v, 3, padding=1).view(n, ch, 9, h, w)
        lo = nb.amin(2).repeat_interleave(8, -2).repeat_interleave(8, -1)
        hi = nb.amax(2).repeat_interleave(8, -2).repeat_interleave(8, -1)
        tol = 16 * 2.0 ** -24 * float(nb.abs().max())
        assert bool((up >= lo - tol).all()) and bool((up <= hi + tol).all())
    # and they are the right combinations (the float64 restatement, float32 rounding of the sums)
    np.testing.assert_allclose(flow_up.numpy(), ref_flow.numpy(), atol=1e-5)
    np.testing.assert_allclose(occ_up.numpy(), ref_occ.numpy(), atol=1e-6)


def test_convex_upsample_error_codes_launch_nothing():
    from scflow_amd import _lib
    lib = _lib.load()
    n, h, w = 1, 2, 3
    c = _case(n, h, w, True, True, 576, seed=1)
    lg, lr, dl, oc = (c[k].cuda() for k in ("logits", "lr", "delta", "occ"))
    fb, flow_up = _guarded((n, 2, 8 * h, 8 * w))
    ob, occ_up = _guarded((n, 1, 8 * h, 8 * w))
    st = torch.cuda.current_stream().cuda_stream

    def call(logits=lg.data_ptr(), lrp=lr.data_ptr(), fu=flow_up.data_ptr(), scale=8, grid=3):
        return lib.scflow_convex_upsample(logits, 576, lrp, dl.data_ptr(), oc.data_ptr(), fu,
                                          occ_up.data_ptr(), None, 0, None, 0, n, h, w, scale, grid,
                                          0.25, 8.0, st)
    assert call(scale=4) == -2 and call(grid=5) == -2          # SCFLOW_EUNSUPPORTED
    assert call(logits=None) == -1 and call(lrp=None) == -1 and call(fu=None) == -1  # SCFLOW_EINVAL
    assert call(fu=flow_up.data_ptr() + 4) == -3               # SCFLOW_EALIGN
    torch.cuda.synchronize()
    assert bool(torch.isnan(fb).all()) and bool(torch.isnan(ob).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(flow_up).all()) and bool(torch.isfinite(occ_up).all())


def test_flow_add_is_exact():
    from scflow_amd import ops
    from scflow_amd.ops import Chan
    n, h, w = 2, 5, 7
    c = _case(n, h, w, True, False, 576, seed=4)
    b0, out0 = _guarded((n * h * w, 2))
    b1, out1 = _guarded((n * h * w, 384))
    ops.flow_add(c["lr"].cuda(), c["delta"].cuda(), Chan.whole(out0), n, h, w, out1=Chan(out1, 382, 2))
    torch.cuda.synchronize()
    assert _untouched(b0) and _untouched(b1)
    want = c["lr"] + c["delta"]
    assert torch.equal(out0.cpu(), want) and torch.equal(out1[:, 382:].cpu(), want)
    assert bool(torch.isnan(out1[:, :382]).all())


def test_library_op_opcheck_and_values():
    from scflow_amd import library  # noqa: F401  (registers the op)
    g = torch.Generator().manual_seed(21)
    n, h, w = 2, 5, 7
    flow = (torch.rand(n, 2, h, w, generator=g) - 0.5) * 6
    logits = torch.randn(n, 576, h, w, generator=g) * 8
    occ = torch.rand(n, 1, h, w, generator=g)
    args = (flow.cuda(), logits.cuda(), occ.cuda(), 0.25, 8.0)
    torch.library.opcheck(torch.ops.scflow.convex_upsample.default, args)
    torch.library.opcheck(torch.ops.scflow.convex_upsample.default,
                          (flow.cuda(), logits.cuda(), None, 0.25, 8.0))
    up, ou = torch.ops.scflow.convex_upsample(*args)
    np.testing.assert_allclose(up.cpu().numpy(), rr.convex_upsample(flow, logits, 0.25, 8.0).numpy(),
                               atol=1e-5)
    np.testing.assert_allclose(ou.cpu().numpy(), rr.convex_upsample(occ, logits, 0.25, 1.0).numpy(),
                               atol=1e-6)
    up2, ou2 = torch.ops.scflow.convex_upsample(flow.cuda(), logits.cuda(), None, 0.25, 8.0)
    assert torch.equal(up2, up) and ou2.numel() == 0
