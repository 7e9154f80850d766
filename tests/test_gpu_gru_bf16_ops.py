"""GPU: the bf16 direct 1×5 / 5×1 conv (SCFLOW_CONV_BF16, conv_sep_bf16.h) launch by launch.

* exact case: small integers × sparse {0, ±1, ±½} weights, quarter-integer bias and bias map —
  every product and partial sum is exact in fp32 (and the operands in bf16), so the plain
  epilogue equals the fp64 restatement BITWISE: tap, channel and lane-map permutations cannot hide
  under a tolerance;
* the GRU epilogues on test_conv_gru_epilogues' data against fp64 on the bf16-rounded operands,
  at the tolerances the project grants a direct fp32 conv of this depth (the products are exact,
  the accumulation is fp32: only the summation order differs);
* reproducibility and refusal.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import gru_bf16_restatement as gr

pytestmark = pytest.mark.gpu

DIRS = [((1, 5), (0, 2)), ((5, 1), (2, 0))]
HXC = 388  # channels of the strided cases' shared buffer (a pixel stride must be 16-B aligned:
#            386 floats is refused with SCFLOW_EALIGN, test_refusals)


@pytest.fixture(scope="module")
def ops():
    from scflow_amd import ops as _ops
    return _ops


def nchw(t2, n, h, w):
    return t2.view(n, h, w, -1).permute(0, 3, 1, 2)


def rows(t4):
    n, c, h, w = t4.shape
    return t4.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def close(a, b, atol, rtol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    print(f"{what}: max err {err.max().item():.3e}")
    assert not bad.any(), f"{what}: max err {err.max().item():.3e} at {bad.nonzero()[0].tolist()}"


def bf16_runner(conv, act=None):
    from scflow_amd import _lib
    from scflow_amd.modules import ConvRunner
    r = ConvRunner([conv.cuda()], act)
    r.fmt = _lib.CONV_BF16
    return r


def sources(ops, x0, x1, strided):
    """src0 / src1 Chans over NCHW x0 / x1 (x1 may be None): contiguous tensors, or channel
    slices of one HXC-channel buffer (src0 at its start, src1 at its end, garbage between)."""
    n, c0, h, w = x0.shape
    if not strided:
        return (ops.Chan.whole(rows(x0).cuda()),
                None if x1 is None else ops.Chan.whole(rows(x1).cuda()))
    buf = torch.full((n * h * w, HXC), 7.75, device="cuda")
    off0 = 0 if x1 is not None else 4
    buf[:, off0:off0 + c0] = rows(x0).cuda()
    if x1 is None:
        return ops.Chan(buf, off0, c0), None
    c1 = x1.shape[1]
    buf[:, HXC - c1:] = rows(x1).cuda()
    return ops.Chan(buf, 0, c0), ops.Chan(buf, HXC - c1, c1)


# ------------------------------------------------------------------------------------ exact case
EXACT_SHAPES = [(1, 4, 32), (2, 32, 32), (1, 8, 64)]
EXACT_SPLITS = [(128, 128, 96), (384, 0, 256), (128, 256, 128)]  # (c0, c1, cout)


def exact_case(ops, k, pad, n, h, w, c0, c1, cout):
    g = torch.Generator().manual_seed(100 * n + h + c1)
    x = torch.randint(-8, 9, (n, c0 + c1, h, w), generator=g).float()
    conv = torch.nn.Conv2d(c0 + c1, cout, k, padding=pad)
    with torch.no_grad():
        vals = torch.tensor([1.0, -1.0, 0.5, -0.5])
        wgt = vals[torch.randint(0, 4, conv.weight.shape, generator=g)]
        wgt = wgt * (torch.rand(conv.weight.shape, generator=g) < 0.06)
        conv.weight.copy_(wgt)
        conv.bias.copy_(torch.randint(-8, 9, (cout,), generator=g).float() / 4)
    bmap = torch.randint(-16, 17, (n, cout, h, w), generator=g).float() / 4
    # fp64 restatement; the operands are bf16 values already, so rounding them is the identity
    assert torch.equal(gr.round_bf16(x), x) and torch.equal(gr.round_bf16(conv.weight.detach()), conv.weight)
    ref = gr.pre_activation(x, conv.weight.detach(), conv.bias.detach(), bmap, pad)
    assert torch.equal(ref.float().double(), ref) and ref.abs().max() > 8  # exact in fp32, not trivial
    dbm = rows(bmap).cuda()
    runner = bf16_runner(conv)
    for strided in (False, True):
        s0, s1 = sources(ops, x[:, :c0], x[:, c0:] if c1 else None, strided)
        out = torch.full((n * h * w, cout + 4), -5.0, device="cuda")
        runner.run(s0, ops.Chan(out, 4, cout), n, h, w, src1=s1, bias_map=ops.Chan.whole(dbm))
        got = ops.chan_to_nchw(ops.Chan(out, 4, cout), n, h, w).cpu()
        assert (out[:, :4] == -5).all()
        assert torch.equal(got, ref.float()), \
            f"strided={strided}: {(got != ref.float()).sum().item()} of {got.numel()} differ, " \
            f"first at {(got != ref.float()).nonzero()[0].tolist()}"


@pytest.mark.parametrize("k,pad", DIRS)
@pytest.mark.parametrize("n,h,w", EXACT_SHAPES)
@pytest.mark.parametrize("c0,c1,cout", EXACT_SPLITS)
def test_exact_case_is_bitwise(ops, k, pad, n, h, w, c0, c1, cout):
    exact_case(ops, k, pad, n, h, w, c0, c1, cout)


@pytest.mark.parametrize("k,pad", DIRS)
def test_exact_case_is_bitwise_with_128_channel_workgroups(ops, k, pad):
    """B = 32 at 32×32 with 256 output channels: 512 workgroups of 128 channels, the grid from
    which the launch takes the 128-channel instantiation (below it, 64-channel workgroups)."""
    exact_case(ops, k, pad, 32, 32, 32, 128, 128, 256)


# ------------------------------------------------------------------------------------ GRU epilogues
# (32, 32, 32): the z|r launch's grid reaches two 128-channel workgroups per CU and takes that
# instantiation; up to (16, 32, 32) every launch runs 64-channel workgroups
GATE_SHAPES = [(1, 4, 32), (2, 32, 32), (16, 32, 32), (1, 64, 64), (32, 32, 32)]


def gru_case(n, h, w, k, pad, hoisted):
    """test_conv_gru_epilogues' data recipe: hoisted → x is the 128 motion channels and a bias
    map carries the context's share; else x is the full 256 channels and there is no map."""
    hc, xc = 128, 128 if hoisted else 256
    g = torch.Generator().manual_seed(11)
    hid = torch.tanh(torch.randn(n * h * w, hc, generator=g))
    x = torch.randn(n * h * w, xc, generator=g)
    bmap = torch.randn(n * h * w, 3 * hc, generator=g) * 0.3 if hoisted else None
    czr = torch.nn.Conv2d(hc + xc, 2 * hc, k, padding=pad)
    cq = torch.nn.Conv2d(hc + xc, hc, k, padding=pad)
    for c in (czr, cq):
        with torch.no_grad():
            c.weight.copy_(torch.randn(c.weight.shape, generator=g) / np.sqrt(c.weight[0].numel()))
            c.bias.copy_(torch.randn(c.bias.shape, generator=g) * 0.1)
    return hid, x, bmap, czr, cq


def run_gru(ops, n, h, w, hid, x, bmap, czr, cq, hoisted):
    """The two launches as ConvGRU.step issues them; returns device (z, r·h, h') as NCHW."""
    from scflow_amd._lib import EPI_GRU_Q, EPI_GRU_ZR
    hc, M = 128, n * h * w
    gate = torch.empty(M, hc, device="cuda")
    rh = torch.empty(M, hc, device="cuda")
    rz, rq = bf16_runner(czr), bf16_runner(cq)
    C = ops.Chan
    if hoisted:
        dh, dx, db = hid.cuda(), x.cuda(), bmap.cuda()
        hidc = C.whole(dh)
        rz.run(hidc, None, n, h, w, src1=C.whole(dx), epilogue=EPI_GRU_ZR, gate=C.whole(gate),
               rh=C.whole(rh), hid=hidc, bias_map=C(db, 0, 2 * hc))
        z_dev, rh_dev = gate.clone(), rh.clone()
        rq.run(C.whole(rh), None, n, h, w, src1=C.whole(dx), epilogue=EPI_GRU_Q, gate=C.whole(gate),
               hid=hidc, bias_map=C(db, 2 * hc, hc))
    else:  # full width: z|r reads one 384-channel source, q reads r·h and HX's x channels
        hx = torch.cat([hid, x], 1).cuda()
        hidc = C(hx, 0, hc)
        rz.run(C.whole(hx), None, n, h, w, epilogue=EPI_GRU_ZR, gate=C.whole(gate), rh=C.whole(rh),
               hid=hidc)
        z_dev, rh_dev = gate.clone(), rh.clone()
        rq.run(C.whole(rh), None, n, h, w, src1=C(hx, hc, x.shape[1]), epilogue=EPI_GRU_Q,
               gate=C.whole(gate), hid=hidc)
    torch.cuda.synchronize()
    return (nchw(z_dev.cpu(), n, h, w), nchw(rh_dev.cpu(), n, h, w),
            ops.chan_to_nchw(hidc, n, h, w).cpu())


@pytest.mark.parametrize("k,pad", DIRS)
@pytest.mark.parametrize("n,h,w", GATE_SHAPES)
@pytest.mark.parametrize("hoisted", [True, False])
def test_gru_epilogues(ops, k, pad, n, h, w, hoisted):
    """z, r·h and h' against fp64 on the bf16-rounded operands: atol 2e-5 / 2e-5 / 3e-5, rtol 1e-5
    (tests/test_gpu_ops.py's for the direct fp32 conv).  Largest errors seen on an MI355X over
    these cases: z 4.0e-7, r·h 3.7e-7, h' 9.5e-7; against the unrounded result 2.5e-3, 2.2e-3, 7.3e-3."""
    hc = 128
    hid, x, bmap, czr, cq = gru_case(n, h, w, k, pad, hoisted)
    z_dev, rh_dev, h_dev = run_gru(ops, n, h, w, hid, x, bmap, czr, cq, hoisted)
    H, X = nchw(hid, n, h, w), nchw(x, n, h, w)
    bzr = None if bmap is None else nchw(bmap[:, :2 * hc], n, h, w)
    bq = None if bmap is None else nchw(bmap[:, 2 * hc:], n, h, w)
    z, rh = gr.zr_launch(H, X, czr.weight.detach().cpu(), czr.bias.detach().cpu(), bzr, pad)
    close(z_dev, z, 2e-5, 1e-5, "z")
    close(rh_dev, rh, 2e-5, 1e-5, "r·h")
    href = gr.q_launch(rh_dev, X, cq.weight.detach().cpu(), cq.bias.detach().cpu(), bq, z_dev, H, pad)
    close(h_dev, href, 3e-5, 1e-5, "h")
    if (n, h, w) == (2, 32, 32):  # negative control: the unrounded fp64 result is far away
        zu, rhu = gr.zr_launch(H, X, czr.weight.detach().cpu(), czr.bias.detach().cpu(), bzr, pad,
                               rounded=False)
        hu = gr.q_launch(rhu.float(), X, cq.weight.detach().cpu(), cq.bias.detach().cpu(), bq,
                         zu.float(), H, pad, rounded=False)
        for what, dev, un, atol in (("z", z_dev, zu, 2e-5), ("r·h", rh_dev, rhu, 2e-5), ("h", h_dev, hu, 3e-5)):
            excess = ((dev.double() - un).abs() - 10 * (atol + 1e-5 * un.abs())).max().item()
            print(f"unrounded {what}: max |dev − fp64| {(dev.double() - un).abs().max().item():.3e}")
            assert excess > 0, f"{what}: the device result is within 10× tolerance of the unrounded one"


@pytest.mark.parametrize("k,pad", DIRS)
def test_plain_epilogue_relu(ops, k, pad):
    """Plain epilogue with bias, ReLU and ``out`` as a channel slice, two sources, cout = 96 (the
    second 64-channel workgroup half empty)."""
    n, h, w, c0, c1, cout = 2, 8, 32, 64, 32, 96
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, c0 + c1, h, w, generator=g)
    conv = torch.nn.Conv2d(c0 + c1, cout, k, padding=pad)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / np.sqrt(conv.weight[0].numel()))
        conv.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    ref = torch.relu(gr.pre_activation(x, conv.weight.detach(), conv.bias.detach(), None, pad))
    s0, s1 = sources(ops, x[:, :c0], x[:, c0:], True)
    out = torch.full((n * h * w, cout + 8), -5.0, device="cuda")
    bf16_runner(conv, "ReLU").run(s0, ops.Chan(out, 4, cout), n, h, w, src1=s1)
    assert (out[:, :4] == -5).all() and (out[:, 4 + cout:] == -5).all()
    close(ops.chan_to_nchw(ops.Chan(out, 4, cout), n, h, w), ref, 2e-5, 1e-5, "relu(conv)")
    assert (ref == 0).any() and (ref > 0).any()


def test_two_runs_are_bitwise_equal(ops):
    n, h, w = 16, 32, 32
    k, pad = DIRS[0]
    hid, x, bmap, czr, cq = gru_case(n, h, w, k, pad, True)
    a = run_gru(ops, n, h, w, hid, x, bmap, czr, cq, True)
    b = run_gru(ops, n, h, w, hid, x, bmap, czr, cq, True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_refusals(ops):
    """An unsupported shape raises ScflowError before anything is launched: the output keeps its
    fill.  (3×3; c0 = 130 cannot even be packed; a 386-float pixel stride is misaligned.)"""
    from scflow_amd import _lib
    from scflow_amd._lib import ScflowError
    n, h, w = 1, 8, 32
    out = torch.full((n * h * w, 64), -5.0, device="cuda")
    src = torch.zeros(n * h * w, 128, device="cuda")
    with pytest.raises(ScflowError):  # 3×3 has no bf16 packing
        bf16_runner(torch.nn.Conv2d(128, 64, 3, padding=1)).run(ops.Chan.whole(src), ops.Chan.whole(out), n, h, w)
    with pytest.raises(ScflowError):  # c0 = 130
        bf16_runner(torch.nn.Conv2d(130, 64, (1, 5), padding=(0, 2))).run(
            ops.Chan.whole(torch.zeros(n * h * w, 130, device="cuda")), ops.Chan.whole(out), n, h, w)
    conv = torch.nn.Conv2d(128, 64, (1, 5), padding=(0, 2)).cuda()
    packed = ops.pack_conv_weight(conv.weight.detach(), 128, 0, w, 1, _lib.CONV_BF16)
    with pytest.raises(ScflowError):  # width 48
        ops.conv2d(ops.Chan.whole(torch.zeros(n * h * 48, 128, device="cuda")), packed, None, n, h, 48,
                   64, 1, 5, 0, 2, out=ops.Chan.whole(torch.empty(n * h * 48, 64, device="cuda")),
                   bk=_lib.CONV_BF16)
    wide = torch.zeros(n * h * w, 386, device="cuda")
    with pytest.raises(ScflowError):  # pixel stride 386 floats: not 16-byte aligned
        ops.conv2d(ops.Chan(wide, 0, 128), packed, None, n, h, w, 64, 1, 5, 0, 2,
                   out=ops.Chan.whole(out), bk=_lib.CONV_BF16)
    a = ops.conv2d_args(ops.Chan.whole(src), packed, None, n, h, w, 64, 1, 5, 0, 2,
                        out=ops.Chan.whole(out), bk=_lib.CONV_BF16)
    a.stride = 2
    assert _lib.load().scflow_conv2d(ctypes.byref(a), ops.raw_stream(0)) == -2  # SCFLOW_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (out == -5).all()
