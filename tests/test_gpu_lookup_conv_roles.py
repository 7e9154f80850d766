"""GPU: the fused lookup + corr_net.0 kernel (scflow_corr_lookup_conv1x1, two wave roles: lookup
producers beside MFMA consumers) against the two launches it replaces.

The A tile is the tiled lookup's own arithmetic and the MFMA order is the wide 1×1 kernel's, so
every comparison with ``tiled lookup + conv2d(bk=CONV_1X1W)`` is exact (torch.equal after
nan_to_num); only the fp64 check has a tolerance (the existing fused test's 1e-4 + 1e-5·|ref|).
Shapes are the smallest the kernel accepts (h, w multiples of 32: no partial workgroup exists).

Without align_corners the tiled lookup refuses the two non-square shapes (a level is 8 wide or tall:
ops.tiled_lookup_ok), so that reference does not exist there.  Those cases assert the refusal and
compare with the row-major lookup instead — the kernel the tiled lookup is itself pinned to, bit
for bit, by test_corr_lookup_tiled_far_out_of_bounds — on the pixels whose flow is finite (the
row-major kernel used at these sizes returns NaN for a non-finite flow where the tiled lookup and
the fused kernel return zeros).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 32), (2, 32, 64), (1, 64, 32)]


@pytest.fixture(scope="module")
def ops():
    from scflow_amd import ops as o
    return o


def edge_flow(n, h, w, g):
    """test_corr_lookup_tiled_far_out_of_bounds' flow patterns, all in image 0 (n may be 1): far
    off the map (±1e4, 1e9), a 0.125-step ramp (windows straddle the map edges at every tile
    phase), h - 0.5, NaN / Inf, zero flow (integer coordinates) and random ±1.5·h."""
    flow = (torch.rand(n, 2, h, w, generator=g) - 0.5) * 3 * h
    flow[0, 0, :4] = 1e4
    flow[0, 1, 4:8] = -1e4
    flow[0, :, 8:16] = torch.arange(8 * w * 2, dtype=torch.float32).view(2, 8, w) * 0.125 - 32
    flow[0, :, 16:20] = float(h) - 0.5
    flow[0, 0, 20, :8] = float("nan")
    flow[0, 1, 20, 8:16] = float("inf")
    flow[0, :, 20, 16:] = 0.0
    flow[0, 0, 21, :16] = 1e9
    flow[0, 1, 21, 16:] = -1e9
    flow[0, :, 22:26] = 0.0
    return flow.permute(0, 2, 3, 1).reshape(-1, 2).contiguous().cuda()


@functools.lru_cache(maxsize=None)
def scene(n, h, w):
    """Per shape, computed once and left unchanged: tiled pyramid, flow, mask (random in [0, 1]
    with exact 0 and 1 entries)."""
    from scflow_amd import ops
    g = torch.Generator().manual_seed(100 * n + h + w)
    f1 = torch.randn(n, 32, h, w, generator=g).cuda()
    f2 = torch.randn(n, 32, h, w, generator=g).cuda()
    pyr = ops.corr_pyramid_tiled(f1, f2, 4)
    _, lv = ops.corr_pyramid(f1, f2, 4)
    buf = ops.pyramid_buffer(lv, n, h, w)
    flow = edge_flow(n, h, w, g)
    mask = torch.rand(n * h * w, generator=g)
    mask[::7] = 0.0
    mask[3::11] = 1.0
    return pyr, flow, mask.cuda(), buf


@functools.lru_cache(maxsize=None)
def layer(cout, act):
    from scflow_amd.modules import ConvRunner
    g = torch.Generator().manual_seed(7 + cout)
    conv = torch.nn.Conv2d(324, cout, 1).cuda()
    with torch.no_grad():
        conv.weight.copy_((torch.randn(cout, 324, 1, 1, generator=g) / 18).cuda())
        conv.bias.copy_((torch.randn(cout, generator=g) * 0.1).cuda())
    return conv, ConvRunner([conv], act)


def both_paths(ops, n, h, w, cout, act, ac, mask, lead=4, tail=0):
    """(fused, separate, corr): outputs in channels [lead, lead + cout) of -3-filled buffers, their
    rows restricted to the pixels the reference covers (all of them with the tiled lookup)."""
    from scflow_amd import _lib
    pyr, flow, _, buf = scene(n, h, w)
    _, r = layer(cout, act)
    packed, bias = r.packed(324, 0, w, _lib.CONV_1X1W)
    M = n * h * w
    corr = torch.empty(M, 324, device="cuda")
    rows = slice(None)
    if ops.tiled_lookup_ok(h, w, 4, 4, ac):
        ops.corr_lookup(pyr, flow, n, h, w, 4, 4, out=ops.Chan.whole(corr), flow_layout="nhwc",
                        align_corners=ac, tiled=True, mask=mask)
    else:
        with pytest.raises(_lib.ScflowError):
            ops.corr_lookup(pyr, flow, n, h, w, 4, 4, out=ops.Chan.whole(corr), flow_layout="nhwc",
                            align_corners=ac, tiled=True, mask=mask)
        ops.corr_lookup(buf, flow, n, h, w, 4, 4, out=ops.Chan.whole(corr), flow_layout="nhwc",
                        align_corners=ac, mask=mask)
        rows = torch.isfinite(flow).all(dim=1)
        assert rows.sum() > 0.9 * M
    sep = torch.full((M, lead + cout + tail), -3.0, device="cuda")
    ops.conv2d(ops.Chan.whole(corr), packed, bias, n, h, w, cout, 1, 1, 0, 0, act,
               out=ops.Chan(sep, lead, cout), bk=_lib.CONV_1X1W)
    fused = torch.full((M, lead + cout + tail), -3.0, device="cuda")
    ops.corr_lookup_conv1x1(pyr, flow, packed, bias, ops.Chan(fused, lead, cout), n, h, w, 4, 4, cout,
                            act=act, align_corners=ac, mask=mask)
    torch.cuda.synchronize()
    return fused[rows], sep[rows], corr[rows]


def same_bits(a, b):
    return torch.equal(torch.nan_to_num(a, nan=123.0), torch.nan_to_num(b, nan=123.0))


@pytest.mark.parametrize("act", ["ReLU", None])
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_fused_roles_bit_identical(ops, n, h, w, ac, act):
    """Fused = tiled lookup + wide 1×1, bit for bit, on zero / ramp / far / non-finite / random
    flows, for both align_corners values, with and without an activation."""
    fused, sep, _ = both_paths(ops, n, h, w, 256, act, ac, None)
    assert same_bits(fused, sep), f"{(fused - sep).abs().nan_to_num().max().item():.3e}"


@pytest.mark.parametrize("act", ["ReLU", None])
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_fused_roles_masked_bit_identical(ops, n, h, w, ac, act):
    """The same with a mask: conv(mask · lookup), the masked tiled lookup's bits."""
    mask = scene(n, h, w)[2]
    fused, sep, _ = both_paths(ops, n, h, w, 256, act, ac, mask)
    assert same_bits(fused, sep), f"{(fused - sep).abs().nan_to_num().max().item():.3e}"
    plain, _, _ = both_paths(ops, n, h, w, 256, act, ac, None)
    assert not same_bits(fused, plain), "the mask changed nothing"


@pytest.mark.parametrize("cout", [256, 96, 40])
def test_fused_roles_narrow_outputs(ops, cout):
    """cout below 256 (idle consumer waves, a half-used 64-channel wave, col ≥ cout masking): the
    slice is exact and the sentinel columns on both sides stay untouched."""
    n, h, w = SHAPES[1]
    fused, sep, _ = both_paths(ops, n, h, w, cout, "ReLU", True, None, lead=4, tail=5)
    assert same_bits(fused[:, 4:4 + cout], sep[:, 4:4 + cout])
    assert (fused[:, :4] == -3).all() and (fused[:, 4 + cout:] == -3).all()
    assert (sep[:, :4] == -3).all() and (sep[:, 4 + cout:] == -3).all()


def test_fused_roles_fp64(ops):
    """The fused output against relu(corr64 @ W64ᵀ + b64) (test_corr_lookup_conv1x1_fused_bit_identical's
    tolerances; rows whose lookup is not finite are compared as NaN-for-NaN by same_bits above)."""
    n, h, w = SHAPES[1]
    fused, _, corr = both_paths(ops, n, h, w, 256, "ReLU", True, None)
    conv, _ = layer(256, "ReLU")
    c64 = corr.double().cpu()
    ref = torch.relu(c64 @ conv.weight.detach().double().cpu().view(256, 324).T +
                     conv.bias.detach().double().cpu())
    ok = torch.isfinite(c64).all(dim=1)
    assert ok.sum() > 0.9 * ok.numel()
    got = fused[:, 4:].double().cpu()
    err = (got[ok] - ref[ok]).abs()
    lim = 1e-4 + 1e-5 * ref[ok].abs()
    assert not (err > lim).any(), f"max err {err.max().item():.3e}"
