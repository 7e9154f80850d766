"""GPU: the occlusion-masked kernels (the reference's mask_corr / mask_flow,
scflow_decoder.py:189-207) — scflow_corr_lookup_masked, scflow_corr_lookup_conv1x1_masked,
scflow_pose_step_masked, scflow_flow_downsample_masked, scflow_corr_lookup_backward_masked and the
``scflow::corr_lookup_masked`` op.

The masks hold exact 0.0 and 1.0 next to random values in (0, 1); the flows hold the far-off-map,
non-finite and edge rows of the unmasked lookup tests.  A masked kernel multiplies where the
unmasked one stores, so its output must equal (unmasked output) · mask bit for bit; equality is
taken after mapping NaN to one value on both sides (a non-finite flow may give NaN samples, and
NaN ≠ NaN), as ``test_corr_lookup_tiled_far_out_of_bounds`` does.
"""
import pytest
import torch

from tests.helpers import golden, t

pytestmark = pytest.mark.gpu
orc = pytest.importorskip("oracle.scflow_oracle")


@pytest.fixture(scope="module")
def ops():
    from scflow_amd import ops as _ops
    return _ops


def same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=123.0), torch.nan_to_num(b, nan=123.0))


def make_mask(m, g):
    """[m] in (0, 1) with exact zeros and ones (every 5th / 7th pixel, and the first two)."""
    mask = torch.rand(m, generator=g) * 0.98 + 0.01
    mask[::5] = 0.0
    mask[3::7] = 1.0
    mask[0], mask[1] = 1.0, 0.0
    return mask


def edge_flow(n, h, w, g):
    """NCHW flows of test_corr_lookup_tiled_far_out_of_bounds: far off the map both ways, a ramp
    over every tile phase, the map edge, zero, NaN and inf rows; other samples random."""
    flow = torch.zeros(n, 2, h, w)
    q = max(h // 8, 1)
    flow[0, 0, :q] = 1e4
    flow[0, 1, q:2 * q] = -1e4
    flow[0, :, 2 * q:4 * q] = torch.arange(2 * q * w * 2, dtype=torch.float32).view(2, 2 * q, w) * 0.125 - h
    flow[0, :, 4 * q:5 * q] = float(h) - 0.5
    flow[0, 0, 5 * q, :w // 4] = float("nan")
    flow[0, 1, 5 * q, w // 4:w // 2] = float("inf")
    for k in range(1, n):
        flow[k] = (torch.rand(2, h, w, generator=g) - 0.5) * 3 * h
    return flow


# ------------------------------------------------------------------------------ lookup
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("radius", [4, 1])
def test_masked_lookup_small_map_golden(ops, radius, ac):
    """n=2, 8×8, L=4 (whole-map LDS regions): the reference fixture's lookup times the mask, at
    the unmasked golden test's tolerance; NCHW and channels-last outputs."""
    gd = golden("ops")
    g = torch.Generator().manual_seed(71)
    _, lv = ops.corr_pyramid(t(gd["pyr_f1"]).cuda(), t(gd["pyr_f2"]).cuda(), 4)
    buf = ops.pyramid_buffer(lv, 2, 8, 8)
    mask = make_mask(2 * 64, g)
    flow = t(gd["lk_flow"]).cuda()
    out = ops.corr_lookup(buf, flow, 2, 8, 8, 4, radius, align_corners=ac, mask=mask.cuda())
    if ac or radius == 4:
        ref = t(gd[f"lk_r{radius}" if ac else "lk_r4_ac0"]) * mask.view(2, 1, 8, 8)
        err = (out.cpu().double() - ref.double()).abs().max().item()
        assert err <= 2e-5 + 2e-5 * ref.abs().max().item(), f"masked lookup vs fixture: {err:.3e}"
    plain = ops.corr_lookup(buf, flow, 2, 8, 8, 4, radius, align_corners=ac)
    assert same(out, plain * mask.cuda().view(2, 1, 8, 8))
    K = 4 * (2 * radius + 1) ** 2
    wide = torch.full((128, K + 8), 7.0, device="cuda")
    ops.corr_lookup(buf, flow.permute(0, 2, 3, 1).contiguous(), 2, 8, 8, 4, radius,
                    out=ops.Chan(wide, 4, K), flow_layout="nhwc", align_corners=ac, mask=mask.cuda())
    assert same(wide[:, 4:4 + K].view(2, 8, 8, K).permute(0, 3, 1, 2), out)
    assert (wide[:, :4] == 7).all() and (wide[:, 4 + K:] == 7).all()


@pytest.mark.parametrize("n,h,w", [(2, 32, 32), (1, 64, 64)])
def test_masked_lookup_lds_and_tiled_bit_identical(ops, n, h, w):
    """The LDS kernel (flat pyramid), the tile-region kernel (tiled, 32×32) and the tile-row kernel
    (tiled, 64×64): masked = (unmasked) · mask, flat = tiled, mask=None = the existing entry — both
    align_corners values, NCHW and channels-last (16-B store path) outputs."""
    g = torch.Generator().manual_seed(72 + h)
    L, r = 4, 4
    K = L * 81
    f1 = torch.randn(n, 16, h, w, generator=g).cuda()
    f2 = torch.randn(n, 16, h, w, generator=g).cuda()
    _, lv = ops.corr_pyramid(f1, f2, L)
    buf = ops.pyramid_buffer(lv, n, h, w)
    tb = ops.corr_pyramid_tiled(f1, f2, L)
    flow = edge_flow(n, h, w, g).cuda()
    fl = flow.permute(0, 2, 3, 1).contiguous()
    mask = make_mask(n * h * w, g).cuda()
    mk = mask.view(n, 1, h, w)
    for ac in (True, False):
        plain = ops.corr_lookup(buf, flow, n, h, w, L, r, align_corners=ac)
        flat = ops.corr_lookup(buf, flow, n, h, w, L, r, align_corners=ac, mask=mask)
        assert same(flat, plain * mk), f"flat, ac={ac}"
        cl = torch.empty(n * h * w, K, device="cuda")
        ops.corr_lookup(buf, fl, n, h, w, L, r, out=ops.Chan.whole(cl), flow_layout="nhwc",
                        align_corners=ac, mask=mask)
        assert same(cl.view(n, h, w, K).permute(0, 3, 1, 2), flat), f"flat channels-last, ac={ac}"
        if not ops.tiled_lookup_ok(h, w, L, r, ac):
            continue
        plain_t = ops.corr_lookup(tb, flow, n, h, w, L, r, align_corners=ac, tiled=True)
        tiled = ops.corr_lookup(tb, flow, n, h, w, L, r, align_corners=ac, tiled=True, mask=mask)
        assert same(tiled, plain_t * mk), f"tiled, ac={ac}"
        assert same(tiled, flat), f"flat vs tiled, ac={ac}"
        ops.corr_lookup(tb, fl, n, h, w, L, r, out=ops.Chan.whole(cl), flow_layout="nhwc",
                        align_corners=ac, tiled=True, mask=mask)
        assert same(cl.view(n, h, w, K).permute(0, 3, 1, 2), flat), f"tiled channels-last, ac={ac}"
    # mask=None through the masked export itself: the existing entry points' bits
    from scflow_amd import _lib
    for pyr, tl in ((buf, 0), (tb, 1)):
        got = torch.empty(n, K, h, w, device="cuda")
        ops._launch("scflow_corr_lookup_masked", flow, pyr.data_ptr(), flow.data_ptr(),
                    _lib.LAYOUT_NCHW, None, got.data_ptr(), _lib.LAYOUT_NCHW, K, n, h, w, L, r, 1, tl)
        assert same(got, ops.corr_lookup(pyr, flow, n, h, w, L, r, tiled=bool(tl))), f"NULL mask, tiled={tl}"


def test_masked_lookup_generic_kernel(ops):
    """L = 5 takes the generic one-thread-per-(pixel, level, column) kernel."""
    g = torch.Generator().manual_seed(75)
    n, h, w, L, r = 2, 32, 48, 5, 2
    f1 = torch.randn(n, 8, h, w, generator=g).cuda()
    f2 = torch.randn(n, 8, h, w, generator=g).cuda()
    buf, _ = ops.corr_pyramid(f1, f2, L)
    flow = edge_flow(n, h, w, g).cuda()
    mask = make_mask(n * h * w, g).cuda()
    plain = ops.corr_lookup(buf, flow, n, h, w, L, r)
    assert same(ops.corr_lookup(buf, flow, n, h, w, L, r, mask=mask), plain * mask.view(n, 1, h, w))


# ------------------------------------------------------------------------------ lookup + 1×1
@pytest.mark.parametrize("n,h,w,seed,far", [(2, 32, 32, 61, False), (3, 32, 64, 62, True),
                                            (1, 64, 64, 63, False)])
def test_masked_lookup_conv1x1_fused_bit_identical(ops, n, h, w, seed, far):
    """scflow_corr_lookup_conv1x1_masked equals the masked tiled lookup followed by the wide 1×1
    conv bit for bit (the producers scale the sample entering the A row, not the accumulator);
    guard columns untouched; mask=None equals the unmasked fused call."""
    from scflow_amd import _lib
    from scflow_amd.modules import ConvRunner
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn(n, 32, h, w, generator=g)
    f2 = torch.randn(n, 32, h, w, generator=g)
    flow = (torch.rand(n, h, w, 2, generator=g) - 0.5) * (4 * h if far else 0.6 * h)
    flow[0, 0, 0] = torch.tensor([float("nan"), 1.0])
    flow[0, 0, 1] = torch.tensor([float("inf"), -2.0])
    flow[0, 1, 0] = torch.tensor([-0.5, -0.5])
    flow[-1, -1, -1] = torch.tensor([1e9, -1e9])
    pyr = ops.corr_pyramid_tiled(f1.cuda(), f2.cuda(), 4)
    fl = flow.reshape(-1, 2).contiguous().cuda()
    M = n * h * w
    mask = make_mask(M, g).cuda()
    conv = torch.nn.Conv2d(324, 256, 1).cuda()
    with torch.no_grad():
        conv.weight.copy_((torch.randn(256, 324, 1, 1, generator=g) / 18).cuda())
        conv.bias.copy_((torch.randn(256, generator=g) * 0.1).cuda())
    packed, bias = ConvRunner([conv], "ReLU").packed(324, 0, w, _lib.CONV_1X1W)
    corr = torch.empty(M, 324, device="cuda")
    ops.corr_lookup(pyr, fl, n, h, w, 4, 4, out=ops.Chan.whole(corr), flow_layout="nhwc", tiled=True,
                    mask=mask)
    sep = torch.full((M, 260), -3.0, device="cuda")
    ops.conv2d(ops.Chan.whole(corr), packed, bias, n, h, w, 256, 1, 1, 0, 0, "ReLU",
               out=ops.Chan(sep, 4, 256), bk=_lib.CONV_1X1W)
    fused = torch.full((M, 260), -3.0, device="cuda")
    ops.corr_lookup_conv1x1(pyr, fl, packed, bias, ops.Chan(fused, 4, 256), n, h, w, 4, 4, 256,
                            mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(fused, sep)
    assert (fused[:, :4] == -3).all()
    # the mask does something: rows with mask 0 are relu(bias), others differ from the unmasked
    plain = torch.full((M, 260), -3.0, device="cuda")
    ops.corr_lookup_conv1x1(pyr, fl, packed, bias, ops.Chan(plain, 4, 256), n, h, w, 4, 4, 256)
    zero = mask == 0
    assert torch.equal(fused[zero][:, 4:], torch.relu(bias).expand(int(zero.sum()), 256))
    assert not torch.equal(fused, plain)
    # NULL mask through the masked export: the unmasked fused call's bits
    null = torch.full((M, 260), -3.0, device="cuda")
    ops._launch("scflow_corr_lookup_conv1x1_masked", fl, pyr.data_ptr(), fl.data_ptr(), None,
                packed.data_ptr(), bias.data_ptr(), ops.Chan(null, 4, 256).ptr, 260, n, h, w, 4, 4,
                256, _lib.SCFLOW_ACT["ReLU"], 1)
    torch.cuda.synchronize()
    assert torch.equal(null, plain)


# ------------------------------------------------------------------------------ pose step
@pytest.mark.parametrize("parts", [3, 2])
@pytest.mark.parametrize("S,s", [(256, 32), (128, 16)])
def test_masked_pose_step(ops, S, s, parts):
    """scflow_pose_step_masked: lr_next and every full-resolution output are the unmasked call's
    bits, lrm_next and hx_next are lr_next · mask_next; without mask_next everything is the
    existing export's."""
    from scflow_amd import synthetic
    n = 3
    sc = synthetic.make_scene(n, S, seed=5)
    R0, t0, K, depth = (t(sc[k]).cuda() for k in ("ref_rotation", "ref_translation", "internel_k",
                                                   "depth"))
    g = torch.Generator().manual_seed(8)
    drot = (torch.tensor([[1.0, 0, 0, 0, 1.0, 0]]).repeat(n, 1) +
            0.03 * torch.randn(n, 6, generator=g)).cuda()
    dt = (0.05 * torch.randn(n, 3, generator=g)).cuda()
    pts = ops.lift_points(depth, K, R0, t0)
    M = n * s * s
    lr = torch.randn(M, 2, generator=g).cuda()
    delta = torch.randn(M, 2, generator=g).cuda()
    mask = torch.rand(M, 1, generator=g).cuda()
    mnext = make_mask(M, g).cuda().view(M, 1)
    scale = float(S // s)

    def run(**kw):
        o = dict(R=torch.full((n, 3, 3), 5.0, device="cuda"), t=torch.full((n, 3), 5.0, device="cuda"),
                 flow=torch.full((n, 2, S, S), 5.0, device="cuda"),
                 up=torch.full((n, 2, S, S), 5.0, device="cuda"),
                 mup=torch.full((n, 1, S, S), 5.0, device="cuda"),
                 nx=torch.full((M, 2), 7.0, device="cuda"), hx=torch.full((M, 6), 7.0, device="cuda"),
                 lrm=torch.full((M, 4), 7.0, device="cuda"))
        if kw.pop("want_lrm", False):
            kw["lrm_next"] = ops.Chan(o["lrm"], 1, 2)
        ops.pose_step(drot, dt, R0, t0, K, pts, o["R"], o["t"], o["flow"], 400.0, lr, delta, mask,
                      o["up"], o["mup"], s, s, scale, lr_next=ops.Chan.whole(o["nx"]),
                      hx_next=ops.Chan(o["hx"], 4, 2), parts=parts, **kw)
        torch.cuda.synchronize()
        return o

    base = run()
    m = run(mask_next=mnext, want_lrm=True)
    for k in ("R", "t", "flow", "up", "mup", "nx"):
        assert torch.equal(m[k], base[k]), k
    want = base["nx"] * mnext
    assert torch.equal(m["lrm"][:, 1:3], want) and torch.equal(m["hx"][:, 4:], want)
    assert (m["lrm"][:, 0] == 7).all() and (m["lrm"][:, 3] == 7).all() and (m["hx"][:, :4] == 7).all()
    assert not torch.equal(want, base["nx"])
    if parts == 2:  # the full-resolution outputs are not written by the ↓8 part
        assert (m["flow"] == 5).all() and (m["up"] == 5).all()
    # no mask: the masked export gives the existing export's bits (lrm_next: a copy of lr_next)
    z = run(want_lrm=True)
    for k in ("R", "t", "flow", "up", "mup", "nx", "hx"):
        assert torch.equal(z[k], base[k]), k
    assert torch.equal(z["lrm"][:, 1:3], base["nx"])
    with pytest.raises(ValueError):  # lrm_next must not alias lr_next
        nx = torch.empty(M, 2, device="cuda")
        ops.pose_step(drot, dt, R0, t0, K, pts, m["R"], m["t"], m["flow"], 400.0, lr, delta, mask,
                      m["up"], m["mup"], s, s, scale, lr_next=ops.Chan.whole(nx),
                      mask_next=mnext, lrm_next=ops.Chan.whole(nx))


def test_masked_pose_step_heads(ops):
    """The masked tail with the pose head's rotation / translation heads in the launch (the
    decoder's default): the unmasked heads export's bits, plus the masked ↓8 outputs."""
    from scflow_amd import synthetic
    n, S, s, k, ncls, split, rch = 3, 256, 32, 256, 21, 4, 6
    sc = synthetic.make_scene(n, S, seed=6)
    R0, t0, K, depth = (t(sc[key]).cuda() for key in ("ref_rotation", "ref_translation",
                                                      "internel_k", "depth"))
    g = torch.Generator().manual_seed(9)
    x = (0.1 * torch.randn(split, n, k, generator=g)).cuda()
    xb = (0.05 * torch.randn(k, generator=g)).cuda()
    Wr = (0.01 * torch.randn(rch * ncls, k, generator=g)).cuda()
    br = torch.tensor([1.0, 0, 0, 0, 1.0, 0] * ncls).cuda()
    Wt = (0.01 * torch.randn(3 * ncls, k, generator=g)).cuda()
    bt = (0.01 * torch.randn(3 * ncls, generator=g)).cuda()
    label = torch.tensor([7, 3, 12], dtype=torch.int64).cuda()
    heads = (x, split, xb, k, Wr, br, rch, Wt, bt, label, ncls)
    pts = ops.lift_points(depth, K, R0, t0)
    M = n * s * s
    lr = torch.randn(M, 2, generator=g).cuda()
    delta = torch.randn(M, 2, generator=g).cuda()
    mask = torch.rand(M, 1, generator=g).cuda()
    mnext = make_mask(M, g).cuda()
    res = []
    for kw in ({}, dict(mask_next=mnext)):
        o = [torch.full(sh, 5.0, device="cuda") for sh in ((n, rch), (n, 3), (n, 3, 3), (n, 3),
                                                           (n, 2, S, S), (n, 2, S, S), (n, 1, S, S),
                                                           (M, 2), (M, 2), (M, 2))]
        if kw:
            kw["lrm_next"] = ops.Chan.whole(o[9])
        ops.pose_step(o[0], o[1], R0, t0, K, pts, o[2], o[3], o[4], 400.0, lr, delta, mask, o[5], o[6],
                      s, s, 8.0, lr_next=ops.Chan.whole(o[7]), hx_next=ops.Chan.whole(o[8]), heads=heads,
                      **kw)
        torch.cuda.synchronize()
        res.append(o)
    a, b = res
    for i in range(8):
        assert torch.equal(a[i], b[i]), i
    assert torch.equal(b[8], a[7] * mnext.view(M, 1)) and torch.equal(b[9], b[8])
    assert torch.equal(a[8], a[7])


def test_masked_flow_downsample(ops):
    """scflow_flow_downsample_masked (the unfused tail under mask_flow): out0 the unmasked call's
    bits, out1 / outm = out0 · mask."""
    g = torch.Generator().manual_seed(12)
    n, S, s = 2, 100, 13
    flow = (torch.randn(n, 2, S, S, generator=g) * 5).cuda()
    M = n * s * s
    mask = make_mask(M, g).cuda()
    a, a1 = torch.empty(M, 2, device="cuda"), torch.zeros(M, 6, device="cuda")
    ops.flow_downsample(flow, ops.Chan.whole(a), s, s, 0.125, out1=ops.Chan(a1, 4, 2))
    b, b1, bm = torch.empty(M, 2, device="cuda"), torch.zeros(M, 6, device="cuda"), torch.empty(M, 2, device="cuda")
    ops.flow_downsample(flow, ops.Chan.whole(b), s, s, 0.125, out1=ops.Chan(b1, 4, 2), mask=mask,
                        outm=ops.Chan.whole(bm))
    assert torch.equal(a, b)
    assert torch.equal(bm, a * mask.view(M, 1)) and torch.equal(b1[:, 4:], bm) and (b1[:, :4] == 0).all()
    c1, cm = torch.zeros(M, 6, device="cuda"), torch.empty(M, 2, device="cuda")
    ops.flow_downsample(flow, ops.Chan.whole(b), s, s, 0.125, out1=ops.Chan(c1, 4, 2),
                        outm=ops.Chan.whole(cm))
    assert torch.equal(c1, a1) and torch.equal(cm, a)


# ------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("radius,flow_kind", [(4, "rand"), (1, "rand"), (4, "grid")])
def test_masked_lookup_backward(ops, radius, flow_kind):
    """The masked lookup's adjoint with respect to the pyramid against fp64 autograd of
    ``orc.corr_lookup(...) * mask`` (test_corr_lookup_backward's set-up and tolerances), and bit
    for bit against the unmasked backward fed ``dout * mask`` — the window kernel is the only
    writer of each map and sums in a fixed order, so the scatter is deterministic."""
    from scflow_amd.train.functions import corr_lookup
    g = torch.Generator().manual_seed(2 + radius)
    n, c, h, w = 2, 16, 16, 16
    f1 = torch.randn(n, c, h, w, generator=g)
    f2 = torch.randn(n, c, h, w, generator=g)
    levels = [lv.double().requires_grad_() for lv in orc.corr_pyramid(f1.double(), f2.double(), 4)]
    flow = (torch.rand(n, 2, h, w, generator=g) - 0.5) * 12
    if flow_kind == "grid":
        d = torch.tensor([1., 2., 4., 8.])[torch.randint(0, 4, (n, 2, h, w), generator=g)]
        flow = torch.round(flow * d) / d
        flow[:, :, ::3] = 0.0
    mask = make_mask(n * h * w, g)
    out = orc.corr_lookup(levels, flow.double(), radius) * mask.double().view(n, 1, h, w)
    gout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * gout).sum().backward()
    bufs = [lv.detach().float().cuda() for lv in levels]
    pyr = ops.pyramid_buffer(bufs, n, h, w).requires_grad_()
    fl = flow.permute(0, 2, 3, 1).contiguous().cuda()
    o = corr_lookup(pyr, fl, n, h, w, 4, radius, mask=mask.cuda())
    err = (o.permute(0, 3, 1, 2).double().cpu() - out.detach()).abs().max().item()
    assert err <= 1e-5 + 1e-5 * out.detach().abs().max().item(), f"masked forward: {err:.3e}"
    go = gout.float().permute(0, 2, 3, 1).contiguous().cuda()
    (o * go).sum().backward()
    torch.cuda.synchronize()
    ref = torch.cat([lv.grad.float().reshape(-1) for lv in levels])
    err = (pyr.grad.double().cpu() - ref.double()).abs().max().item()
    assert err <= 1e-5 + 1e-5 * ref.abs().max().item(), f"masked backward: {err:.3e}"
    # the unmasked backward fed dout · mask, and the NULL-mask call
    K = 4 * (2 * radius + 1) ** 2
    dm = (go.view(n * h * w, K) * mask.cuda().view(-1, 1)).contiguous()
    want = torch.zeros_like(pyr.grad)
    ops.corr_lookup_backward(dm, fl, want, n, h, w, 4, radius)
    assert torch.equal(pyr.grad, want)
    from scflow_amd import _lib
    a, b = torch.zeros_like(want), torch.zeros_like(want)
    d = go.view(n * h * w, K)
    ops.corr_lookup_backward(d, fl, a, n, h, w, 4, radius)
    ops._launch("scflow_corr_lookup_backward_masked", d, d.data_ptr(), _lib.LAYOUT_NHWC, K,
                fl.data_ptr(), _lib.LAYOUT_NHWC, None, b.data_ptr(), n, h, w, 4, radius)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------ torch.library
def test_opcheck_corr_lookup_masked():
    from scflow_amd import library
    g = torch.Generator().manual_seed(51)
    n, c, h, w = 2, 16, 16, 16
    f1 = torch.randn(n, c, h, w, generator=g).cuda()
    f2 = torch.randn(n, c, h, w, generator=g).cuda()
    flow = ((torch.rand(n, 2, h, w, generator=g) - 0.5) * 10).cuda()
    mask = make_mask(n * h * w, g).view(n, 1, h, w).cuda()
    pyr = library.corr_pyramid(f1, f2, 4)
    torch.library.opcheck(torch.ops.scflow.corr_lookup_masked.default,
                          (pyr.detach().clone().requires_grad_(), flow, mask, 4, 4, True))
    torch.library.opcheck(torch.ops.scflow.corr_lookup_masked.default, (pyr, flow, mask, 4, 1, False))
    out = torch.ops.scflow.corr_lookup_masked(pyr, flow, mask, 4, 4, True)
    assert same(out, torch.ops.scflow.corr_lookup(pyr, flow, 4, 4, True) * mask)
    # no gradient for the mask or the flow: an attached one is an error, not a silent zero
    p = pyr.detach().clone().requires_grad_()
    for fl, mk in ((flow, mask.clone().requires_grad_()), (flow.clone().requires_grad_(), mask)):
        o = torch.ops.scflow.corr_lookup_masked(p, fl, mk, 4, 4, True)
        with pytest.raises(NotImplementedError):
            o.sum().backward()
