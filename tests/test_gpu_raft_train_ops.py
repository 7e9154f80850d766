"""GPU: scflow_convex_upsample_bwd (the adjoint of RAFT's convex ×8 upsampling; two launches, no
float atomics) against float64 torch autograd of ``raft_restatement.convex_upsample``.

Bound, per output (dlogits, dx, docc) — the forward test's rule: the kernel's maximum absolute
error is at most 4 × the error of the SAME composition differentiated by torch in float32 on the
same inputs, measured here, with a floor of 16 · 2^-24 · max|reference| for the cases where torch's
float32 happens to be exact.  Sentinel (NaN) bands around every output and the workspace show that
nothing else is written; dlogits channels ≥ 576 stay untouched; two runs agree bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import raft_restatement as rr

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1, 1, 1),    # every neighbour padded
              (2, 2, 3),
              (2, 3, 11),   # a full strip + a 3-pixel tail, a strip boundary inside a row, all four
                            # borders, two samples
              (1, 32, 32)]  # several full strips per row, many workgroups
# (occ given, g_occ given, logit pixel stride ls, dlogits pixel stride dls)
VARIANTS = [(True, True, 576, 576), (True, False, 580, 640), (False, False, 580, 576),
            (True, True, 576, 640)]
PAD = 32  # floats of sentinel before and after each output (keeps 16-byte alignment)
FLOOR = 16 * 2.0 ** -24


def _guarded(shape, dev="cuda"):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), float("nan"), device=dev)
    return buf, buf[PAD:PAD + n].view(*shape)


def _untouched(buf):
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all())


def _case(n, h, w, with_occ, with_gocc, ls, seed, logit_std=8.0):
    g = torch.Generator().manual_seed(seed)
    m = n * h * w
    return dict(logits=torch.randn(m, ls, generator=g) * logit_std,
                x=(torch.rand(m, 2, generator=g) - 0.5) * 6,
                occ=torch.rand(m, 1, generator=g) if with_occ else None,
                g_flow=torch.randn(n, 2, 8 * h, 8 * w, generator=g),
                g_occ=torch.randn(n, 1, 8 * h, 8 * w, generator=g) if with_gocc else None)


def _autograd(c, n, h, w, dtype):
    """torch autograd of the composition in ``dtype`` → (dlogits [m, 576], dx [m, 2], docc [m, 1] or
    None), channels-last like the kernel's outputs."""
    nchw = lambda a: a.view(n, h, w, -1).permute(0, 3, 1, 2).contiguous().to(dtype)  # noqa: E731
    rows = lambda a: a.permute(0, 2, 3, 1).reshape(n * h * w, -1)  # noqa: E731
    lg = nchw(c["logits"][:, :576]).requires_grad_()
    x = nchw(c["x"]).requires_grad_()
    obj = (rr.convex_upsample(x, lg, 0.25, 8.0) * c["g_flow"].to(dtype)).sum()
    occ = None
    if c["occ"] is not None:
        occ = nchw(c["occ"]).requires_grad_()
        up = rr.convex_upsample(occ, lg, 0.25, 1.0)
        # without g_occ the occlusion's gradient is zero (its term drops out)
        obj = obj + (up * (c["g_occ"].to(dtype) if c["g_occ"] is not None else 0.0)).sum()
    obj.backward()
    return rows(lg.grad), rows(x.grad), (None if occ is None else rows(occ.grad))


def _run_kernel(c, n, h, w, ls, dls, call=None):
    """The C entry on guarded buffers → (dlogits [m, dls], dx, docc or None) on the CPU."""
    from scflow_amd import _lib
    lib = _lib.load()
    dev = "cuda"
    m = n * h * w
    with_occ = c["occ"] is not None
    C = 3 if with_occ and c["g_occ"] is not None else 2
    t = {k: (None if v is None else v.to(dev)) for k, v in c.items()}
    lb, dlogits = _guarded((m, dls))
    xb, dx = _guarded((m, 2))
    ob, docc = _guarded((m, 1))
    wb, ws = _guarded((m * 9 * C,))
    p = lambda a: None if a is None else a.data_ptr()  # noqa: E731
    rc = lib.scflow_convex_upsample_bwd(
        p(t["logits"]), ls, p(t["x"]), p(t["occ"]), p(t["g_flow"]), p(t["g_occ"]), p(dlogits), dls,
        p(dx), p(docc) if with_occ else None, p(ws), ws.numel() * 4, n, h, w, 8, 3, 0.25, 8.0,
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for nm, b in (("dlogits", lb), ("dx", xb), ("docc", ob), ("workspace", wb)):
        assert _untouched(b), f"{nm}: written outside the buffer"
    if not with_occ:
        assert bool(torch.isnan(ob).all()), "docc written without occ"
    if dls > 576:
        assert bool(torch.isnan(dlogits[:, 576:]).all()), "dlogits: channels >= 576 written"
    return dlogits.cpu(), dx.cpu(), (docc.cpu() if with_occ else None)


def _check(name, got, ref64, ref32):
    err = float((got.double() - ref64).abs().max())
    f32 = float((ref32.double() - ref64).abs().max())
    bound = max(4 * f32, FLOOR * float(ref64.abs().max()))
    print(f"{name}: kernel max err {err:.3e}, float32 torch {f32:.3e}, bound {bound:.3e}")
    assert err <= bound, name


@pytest.mark.parametrize("variant", VARIANTS,
                         ids=lambda v: f"occ{int(v[0])}-gocc{int(v[1])}-ls{v[2]}-dls{v[3]}")
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "n%d-%dx%d" % g)
def test_convex_upsample_bwd_matches_float64_autograd(geom, variant):
    n, h, w = geom
    with_occ, with_gocc, ls, dls = variant
    c = _case(n, h, w, with_occ, with_gocc, ls, seed=100 * h + w + 7 * ls + dls)
    ref64 = _autograd(c, n, h, w, torch.float64)
    ref32 = _autograd(c, n, h, w, torch.float32)
    got = _run_kernel(c, n, h, w, ls, dls)
    _check("dlogits", got[0][:, :576], ref64[0], ref32[0])
    _check("dx", got[1], ref64[1], ref32[1])
    if with_occ:
        _check("docc", got[2], ref64[2], ref32[2])
        if not with_gocc:
            assert float(got[2].abs().max()) == 0.0
    again = _run_kernel(c, n, h, w, ls, dls)  # bitwise reproducible (NaN sentinels compare equal)
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(torch.nan_to_num(a, nan=-7.0),
                                                        torch.nan_to_num(b, nan=-7.0))


def test_convex_upsample_bwd_large_logits_stay_finite_and_sum_to_zero():
    """Logits of standard deviation 64 (scaled: 16, a nearly one-hot softmax; exp overflows without
    the maximum subtracted): everything stays finite, and since Σ_k w_k = 1 the nine dlogits of a
    (pixel, sub-pixel) sum to zero — up to rounding: nine terms, each within the floor
    16 · 2^-24 · max|reference dlogits|."""
    n, h, w = 2, 3, 11
    c = _case(n, h, w, True, True, 576, seed=9, logit_std=64.0)
    ref64 = _autograd(c, n, h, w, torch.float64)
    dlogits, dx, docc = _run_kernel(c, n, h, w, 576, 576)
    assert all(bool(torch.isfinite(a).all()) for a in (dlogits, dx, docc))
    s = dlogits.view(n * h * w, 9, 64).double().sum(1).abs().max()
    bound = 9 * FLOOR * float(ref64[0].abs().max())
    print(f"|sum_k dlogits| max {float(s):.3e}, bound {bound:.3e}")
    assert float(s) <= bound
    ref32 = _autograd(c, n, h, w, torch.float32)
    _check("dlogits", dlogits, ref64[0], ref32[0])
    _check("dx", dx, ref64[1], ref32[1])
    _check("docc", docc, ref64[2], ref32[2])


def test_convex_upsample_bwd_error_codes_launch_nothing():
    from scflow_amd import _lib
    lib = _lib.load()
    n, h, w = 1, 2, 3
    m = n * h * w
    c = _case(n, h, w, True, True, 576, seed=1)
    t = {k: v.cuda() for k, v in c.items()}
    lb, dlogits = _guarded((m, 576))
    xb, dx = _guarded((m, 2))
    ob, docc = _guarded((m, 1))
    wb, ws = _guarded((m * 27,))
    st = torch.cuda.current_stream().cuda_stream
    base = dict(logits=t["logits"].data_ptr(), ls=576, x=t["x"].data_ptr(), occ=t["occ"].data_ptr(),
                g_flow=t["g_flow"].data_ptr(), g_occ=t["g_occ"].data_ptr(), dlogits=dlogits.data_ptr(),
                dls=576, dx=dx.data_ptr(), docc=docc.data_ptr(), ws=ws.data_ptr(),
                ws_bytes=ws.numel() * 4, n=n, h=h, w=w, scale=8, grid=3)

    def call(**over):
        a = dict(base, **over)
        return lib.scflow_convex_upsample_bwd(
            a["logits"], a["ls"], a["x"], a["occ"], a["g_flow"], a["g_occ"], a["dlogits"], a["dls"],
            a["dx"], a["docc"], a["ws"], a["ws_bytes"], a["n"], a["h"], a["w"], a["scale"], a["grid"],
            0.25, 8.0, st)
    assert call(scale=4) == -2 and call(grid=5) == -2                       # SCFLOW_EUNSUPPORTED
    for k in ("logits", "x", "g_flow", "dlogits", "dx", "ws"):               # SCFLOW_EINVAL
        assert call(**{k: None}) == -1, k
    assert call(ls=575) == -1 and call(dls=575) == -1 and call(n=0) == -1
    assert call(occ=None) == -1                       # g_occ / docc without occ
    assert call(ws_bytes=m * 27 * 4 - 4) == -1        # workspace too small
    assert call(g_flow=base["g_flow"] + 4) == -3 and call(g_occ=base["g_occ"] + 4) == -3  # EALIGN
    torch.cuda.synchronize()
    for b in (lb, xb, ob, wb):
        assert bool(torch.isnan(b).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(a).all()) for a in (dlogits, dx, docc))


def _nchw_case(seed=21, n=2, h=5, w=7):
    g = torch.Generator().manual_seed(seed)
    flow = (torch.rand(n, 2, h, w, generator=g) - 0.5) * 6
    logits = torch.randn(n, 576, h, w, generator=g) * 8
    occ = torch.rand(n, 1, h, w, generator=g)
    g_flow = torch.randn(n, 2, 8 * h, 8 * w, generator=g)
    g_occ = torch.randn(n, 1, 8 * h, 8 * w, generator=g)
    return [a.cuda() for a in (flow, logits, occ, g_flow, g_occ)]


def test_library_ops_opcheck_with_grad():
    from scflow_amd import library  # noqa: F401  (registers the ops)
    flow, logits, occ, g_flow, g_occ = _nchw_case()
    rg = lambda a: a.clone().requires_grad_()  # noqa: E731
    torch.library.opcheck(torch.ops.scflow.convex_upsample.default,
                          (rg(flow), rg(logits), rg(occ), 0.25, 8.0))
    torch.library.opcheck(torch.ops.scflow.convex_upsample.default,
                          (rg(flow), rg(logits), None, 0.25, 8.0))
    torch.library.opcheck(torch.ops.scflow.convex_upsample_backward.default,
                          (g_flow, g_occ, flow, logits, occ, 0.25, 8.0))
    torch.library.opcheck(torch.ops.scflow.convex_upsample_backward.default,
                          (g_flow, None, flow, logits, None, 0.25, 8.0))


@pytest.mark.parametrize("with_occ", [True, False])
def test_library_backward_equals_training_function_bitwise(with_occ):
    """``.backward()`` through torch.ops.scflow.convex_upsample (NCHW operands, layout transposes
    around the kernel) and through train/functions.py convex_upsample (channels-last) are the same
    launch on the same values: equal bit for bit, and right (float64 autograd, 1e-4 relative to
    each gradient's largest magnitude)."""
    from scflow_amd import library  # noqa: F401
    from scflow_amd.train.functions import convex_upsample
    flow, logits, occ, g_flow, g_occ = _nchw_case(seed=22)
    if not with_occ:
        occ = None
    a = [None if t is None else t.clone().requires_grad_() for t in (flow, logits, occ)]
    up, ou = torch.ops.scflow.convex_upsample(a[0], a[1], a[2], 0.25, 8.0)
    ((up * g_flow).sum() + ((ou * g_occ).sum() if with_occ else 0.0)).backward()
    cl = lambda t: None if t is None else t.permute(0, 2, 3, 1).contiguous().requires_grad_()  # noqa: E731
    b = [cl(flow), cl(logits), cl(occ)]
    up2, ou2 = convex_upsample(b[0], b[1], b[2], 0.25, 8.0)
    ((up2 * g_flow).sum() + ((ou2 * g_occ).sum() if with_occ else 0.0)).backward()
    torch.cuda.synchronize()
    assert torch.equal(up, up2) and (not with_occ or torch.equal(ou, ou2))
    assert ou2 is None or with_occ
    r = [None if t is None else t.double().cpu().requires_grad_() for t in (flow, logits, occ)]
    obj = (rr.convex_upsample(r[0], r[1], 0.25, 8.0) * g_flow.double().cpu()).sum()
    if with_occ:
        obj = obj + (rr.convex_upsample(r[2], r[1], 0.25, 1.0) * g_occ.double().cpu()).sum()
    obj.backward()
    for x, y, z in zip(a, b, r):
        if x is None:
            continue
        assert torch.equal(x.grad, y.grad.permute(0, 3, 1, 2))
        assert float((x.grad.double().cpu() - z.grad).abs().max()) <= 1e-4 * float(z.grad.abs().max())
