"""GPU: the bf16 direct 3×3 conv (SCFLOW_CONV_BF16_3X3, conv3_bf16.h) launch by launch, through a
ConvRunner with ``fmt`` set.

* exact case: small integers (they encode sample, row, column and channel) × sparse {0, ±1, ±½}
  weights, quarter-integer bias — every product and partial sum is exact in fp32 (and the operands
  in bf16), so the output equals the fp64 restatement BITWISE: tap, channel-block and lane-map
  permutations, a halo row taken from the neighbouring sample or a wrong zero border cannot hide
  under a tolerance;
* masked stores: 126 channels into a 132-channel buffer, everything else bitwise untouched;
* test_conv2d_variants' random data against fp64 on the bf16-rounded operands, at the tolerance
  the project grants a direct fp32 conv of this depth (the products are exact, the accumulation is
  fp32: only the summation order differs), with the direct fp32 conv on the same rounded operands
  printed beside it, and the unrounded fp64 result as the negative control;
* reproducibility and refusal.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv3_bf16_restatement as cr
from tests.test_gpu_gru_bf16_ops import close, sources

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from scflow_amd import ops as _ops
    return _ops


def runner_for(conv, act=None, fmt="bf16"):
    """A ConvRunner on the bf16 3×3 format, or (``fmt`` 16) on the direct fp32 conv."""
    from scflow_amd import _lib
    from scflow_amd.modules import ConvRunner
    r = ConvRunner([conv.cuda()], act)
    r.fmt = _lib.CONV_BF16_3X3 if fmt == "bf16" else fmt
    return r


# ------------------------------------------------------------------------------------ exact case
# (n, h, w, c0, c1, cout): one row block of one sample and 32 channels; three samples × three row
# blocks with 8 stages and three 64-channel workgroups; W = 64 (two column blocks), two sources, a
# masked last block; 33 channels (a workgroup whose second wave pair has one live channel); 96
# channels (three 32-channel blocks: the second workgroup's second wave pair has no block — like
# the first shape's, it re-reads the last packed block and stores nothing)
EXACT_SHAPES = [(1, 4, 32, 32, 0, 32), (3, 12, 32, 256, 0, 192), (2, 8, 64, 64, 32, 126),
                (2, 8, 32, 32, 0, 33), (2, 8, 32, 64, 0, 96)]
# The launch rule selects one instantiation only (64-channel workgroups), which
# every case here runs.  This one has 512 row × column blocks × two channel blocks = 1024
# workgroups: every workgroup slot of 256 CUs taken, 16 samples, both column blocks of W = 64.
EXACT_FULL_GRID = (16, 64, 64, 32, 0, 126)


def exact_data(n, h, w, c0, c1, cout):
    cin = c0 + c1
    g = torch.Generator().manual_seed(1000 * n + 10 * h + cout)
    ni, ci, yi, xi = torch.meshgrid(torch.arange(n), torch.arange(cin), torch.arange(h), torch.arange(w),
                                    indexing="ij")
    x = ((37 * ni + 13 * yi + 29 * xi + 3 * ci + 11 * (ci // 32)) % 257 - 128).float()
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1)
    with torch.no_grad():
        vals = torch.tensor([1.0, -1.0, 0.5, -0.5])
        wgt = vals[torch.randint(0, 4, conv.weight.shape, generator=g)]
        wgt = wgt * (torch.rand(conv.weight.shape, generator=g) < 0.06)
        conv.weight.copy_(wgt)
        conv.bias.copy_(torch.randint(-8, 9, (cout,), generator=g).float() / 4)
    wd = conv.weight.detach()
    # every (tap, 32-channel block) carries weights, and no two of them the same pattern
    pats = [wd[:, 32 * b:32 * b + 32, ky, kx] for b in range(cin // 32) for ky in range(3) for kx in range(3)]
    assert all(p.abs().sum() > 0 for p in pats)
    assert all(not torch.equal(p, q) for i, p in enumerate(pats) for q in pats[:i])
    assert x.abs().max() <= 128 and torch.equal(cr.round_bf16(x), x) and torch.equal(cr.round_bf16(wd), wd)
    ref = cr.launch(x, wd, conv.bias.detach())
    assert torch.equal(ref.float().double(), ref) and ref.abs().max() > 128  # exact in fp32, not trivial
    return x, conv, ref.float()


def exact_case(ops, n, h, w, c0, c1, cout):
    x, conv, ref = exact_data(n, h, w, c0, c1, cout)
    runner = runner_for(conv)
    for strided in (False, True):
        s0, s1 = sources(ops, x[:, :c0], x[:, c0:] if c1 else None, strided)
        out = torch.full((n * h * w, cout + 7), -5.0, device="cuda")
        runner.run(s0, ops.Chan(out, 4, cout), n, h, w, src1=s1)
        got = ops.chan_to_nchw(ops.Chan(out, 4, cout), n, h, w).cpu()
        assert (out[:, :4] == -5).all() and (out[:, 4 + cout:] == -5).all()
        assert torch.equal(got, ref), \
            f"strided={strided}: {(got != ref).sum().item()} of {got.numel()} differ, " \
            f"first at {(got != ref).nonzero()[0].tolist()}"


@pytest.mark.parametrize("n,h,w,c0,c1,cout", EXACT_SHAPES)
def test_exact_case_is_bitwise(ops, n, h, w, c0, c1, cout):
    exact_case(ops, n, h, w, c0, c1, cout)


def test_exact_case_is_bitwise_on_a_full_grid(ops):
    exact_case(ops, *EXACT_FULL_GRID)


def test_masked_stores_leave_the_neighbouring_channels(ops):
    """out_net's destination: 126 channels in front of the two flow channels of a wider buffer.
    Every bit outside the 126 channels keeps the sentinel, whatever the padded block computes."""
    n, h, w, c0, c1, cout = 2, 8, 64, 64, 32, 126
    x, conv, ref = exact_data(n, h, w, c0, c1, cout)
    s0, s1 = sources(ops, x[:, :c0], x[:, c0:], False)
    for off in (0, 2, 6):
        buf = torch.full((n * h * w, 132), float("nan"), device="cuda")
        before = buf.view(torch.int32).clone()
        runner_for(conv).run(s0, ops.Chan(buf, off, cout), n, h, w, src1=s1)
        torch.cuda.synchronize()
        after = buf.view(torch.int32)
        assert torch.equal(after[:, :off], before[:, :off])
        assert torch.equal(after[:, off + cout:], before[:, off + cout:])
        assert torch.equal(ops.chan_to_nchw(ops.Chan(buf, off, cout), n, h, w).cpu(), ref)


# ------------------------------------------------------------------------------------ tolerance case
TOL_SHAPES = [(2, 32, 32, 256, 0, 192), (2, 32, 32, 192, 64, 126), (1, 64, 64, 128, 0, 64),
              (16, 32, 32, 256, 0, 192)]
_cache = {}


def variants_data(n, h, w, c0, c1, cout, seed=0):
    """tests/test_gpu_ops.py's ``_conv_case`` data recipe; the fp64 pre-activations on the rounded
    and on the unrounded operands, computed once per shape and shared."""
    key = (n, h, w, c0, c1, cout, seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(seed)
        x0 = torch.randn(n, c0, h, w, generator=g)
        x1 = torch.randn(n, c1, h, w, generator=g) if c1 else None
        conv = torch.nn.Conv2d(c0 + c1, cout, 3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / np.sqrt(conv.weight[0].numel()))
            conv.bias.copy_(torch.randn(cout, generator=g) * 0.1)
        xin = torch.cat([x0, x1], 1) if c1 else x0
        wd, bd = conv.weight.detach().clone(), conv.bias.detach().clone()
        _cache[key] = dict(x=xin, w=wd, b=bd, rounded=cr.launch(xin, wd, bd),
                           unrounded=cr.launch(xin, wd, bd, rounded=False))
    return _cache[key]


def tolerance(c0, c1):
    """tests/test_gpu_ops.py's for the direct fp32 conv: atol 2e-6·√K·4, rtol 1e-5, K = 9·(c0 + c1)."""
    return 2e-6 * np.sqrt(9 * (c0 + c1)) * 4, 1e-5


def device_conv(ops, d, n, h, w, c0, c1, cout, act, fmt="bf16", rounded_inputs=False):
    """The launch on the case's fp32 data (or, for the fp32 yardstick, on its bf16-rounded data
    with bf16-rounded weights), sources as channel slices of wider buffers."""
    x = cr.round_bf16(d["x"]) if rounded_inputs else d["x"]
    conv = torch.nn.Conv2d(c0 + c1, cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(cr.round_bf16(d["w"]) if rounded_inputs else d["w"])
        conv.bias.copy_(d["b"])
    s0, s1 = sources(ops, x[:, :c0], x[:, c0:] if c1 else None, True)
    out = torch.full((n * h * w, cout + 3), -5.0, device="cuda")
    runner_for(conv, act, fmt).run(s0, ops.Chan(out, 3, cout), n, h, w, src1=s1)
    assert (out[:, :3] == -5).all()
    return ops.chan_to_nchw(ops.Chan(out, 3, cout), n, h, w).cpu()


@pytest.mark.parametrize("act", [None, "ReLU"])
@pytest.mark.parametrize("n,h,w,c0,c1,cout", TOL_SHAPES)
def test_random_data_within_the_direct_fp32_tolerance(ops, n, h, w, c0, c1, cout, act):
    """Against fp64 on the rounded operands, atol 2e-6·√K·4 (3.84e-4 at K = 2304), rtol 1e-5.
    Largest errors seen on an MI355X over these cases: bf16 kernel 3.3e-6, the direct fp32 conv on
    the same rounded operands 7.7e-6."""
    d = variants_data(n, h, w, c0, c1, cout)
    ref = cr.ACTS[act](d["rounded"])
    atol, rtol = tolerance(c0, c1)
    got = device_conv(ops, d, n, h, w, c0, c1, cout, act)
    # the yardstick: the existing direct fp32 conv (bk = 16) on the same rounded operands
    fp32 = device_conv(ops, d, n, h, w, c0, c1, cout, act, fmt=16, rounded_inputs=True)
    print(f"conv3 ({n},{h},{w},{c0},{c1},{cout}) {act}: direct fp32 conv on the rounded operands, "
          f"max err {(fp32.double() - ref).abs().max().item():.3e}")
    close(got, ref, atol, rtol, f"conv3 ({n},{h},{w},{c0},{c1},{cout}) {act}: bf16 kernel")
    if act == "ReLU":
        assert (ref == 0).any() and (ref > 0).any()


def test_negative_control_the_unrounded_result_is_outside_the_tolerance(ops):
    """The tolerance separates "rounded as specified" from "not rounded": on the CPU alone the two
    fp64 results are further apart than it allows, and so is the device from the unrounded one."""
    n, h, w, c0, c1, cout = TOL_SHAPES[0]
    d = variants_data(n, h, w, c0, c1, cout)
    atol, rtol = tolerance(c0, c1)
    un = d["unrounded"]
    ref_excess = ((d["rounded"] - un).abs() - (atol + rtol * un.abs())).max().item()
    print(f"rounded vs unrounded fp64: max |Δ| {(d['rounded'] - un).abs().max().item():.3e} (atol {atol:.3e})")
    assert ref_excess > 0, "the reference alone does not exceed the tolerance on this data"
    got = device_conv(ops, d, n, h, w, c0, c1, cout, None).double()
    print(f"device vs unrounded fp64: max |Δ| {(got - un).abs().max().item():.3e}")
    assert ((got - un).abs() - (atol + rtol * un.abs())).max().item() > 0


# ------------------------------------------------------------------------------------ the rest
def test_two_runs_are_bitwise_equal(ops):
    n, h, w, c0, c1, cout = TOL_SHAPES[1]
    d = variants_data(n, h, w, c0, c1, cout)
    a = device_conv(ops, d, n, h, w, c0, c1, cout, "ReLU")
    b = device_conv(ops, d, n, h, w, c0, c1, cout, "ReLU")
    assert torch.equal(a, b)


def test_refusals(ops):
    """scflow_conv2d answers −2 (SCFLOW_EUNSUPPORTED) out of the domain and −3 (SCFLOW_EALIGN) for
    a 386-float pixel stride, before anything is launched: the output keeps its fill.  Through a
    ConvRunner the same calls raise ScflowError."""
    from scflow_amd import _lib
    from scflow_amd._lib import ScflowError
    n, h, w = 1, 8, 32
    lib = _lib.load()
    out = torch.full((n * h * w, 64), -5.0, device="cuda")
    src = torch.zeros(n * h * w, 128, device="cuda")
    conv = torch.nn.Conv2d(128, 64, 3, padding=1).cuda()
    packed = ops.pack_conv_weight(conv.weight.detach(), 128, 0, w, 1, _lib.CONV_BF16_3X3)

    def args(s=None, hh=h, ww=w, **over):
        a = ops.conv2d_args(ops.Chan.whole(src) if s is None else s, packed, None, n, hh, ww, 64, 3, 3, 1, 1,
                            out=ops.Chan.whole(out), bk=_lib.CONV_BF16_3X3)
        for k, v in over.items():
            setattr(a, k, v)
        return a
    assert lib.scflow_conv2d(ctypes.byref(args(stride=2)), ops.raw_stream(0)) == -2
    assert lib.scflow_conv2d(ctypes.byref(args(ph=0, pw=0)), ops.raw_stream(0)) == -2
    assert lib.scflow_conv2d(ctypes.byref(args(hh=6)), ops.raw_stream(0)) == -2        # h % 4
    assert lib.scflow_conv2d(ctypes.byref(args(hh=4, ww=48)), ops.raw_stream(0)) == -2  # width 48
    assert lib.scflow_conv2d(ctypes.byref(args(epilogue=_lib.EPI_GRU_Q, gate=out.data_ptr(),
                                               hid=out.data_ptr())), ops.raw_stream(0)) == -2
    wide = torch.zeros(n * h * w, 386, device="cuda")
    assert lib.scflow_conv2d(ctypes.byref(args(ops.Chan(wide, 0, 128))), ops.raw_stream(0)) == -3
    with pytest.raises(ScflowError):  # the same through the runner
        runner_for(conv).run(ops.Chan(wide, 0, 128), ops.Chan.whole(out), n, h, w)
    with pytest.raises(ScflowError):  # c0 = 130 cannot even be packed
        runner_for(torch.nn.Conv2d(130, 64, 3, padding=1)).run(
            ops.Chan.whole(torch.zeros(n * h * w, 130, device="cuda")), ops.Chan.whole(out), n, h, w)
    with pytest.raises(ScflowError):  # 1×5 has no 3×3 packing
        runner_for(torch.nn.Conv2d(128, 64, (1, 5), padding=(0, 2))).run(ops.Chan.whole(src),
                                                                        ops.Chan.whole(out), n, h, w)
    torch.cuda.synchronize()
    assert (out == -5).all()
