"""GPU: the bf16 direct 3×3 conv's RAFT-encoder form (SCFLOW_CONV_BF16_3X3N, conv3_bf16.h), one
launch each through ``ops.conv2d``.

* exact case: integer inputs, power-of-two input scales, integer shifts (positive ones present, so
  that a border pixel computed as relu(in_shift) instead of 0 shows), sparse {0, ±1, ±½} weights,
  quarter-integer bias and output shift, power-of-two output scales, integer residual — every
  intermediate is exact in bf16 and fp32, so the device equals the fp64 restatement BITWISE, from
  contiguous tensors and from channel slices of NaN-filled wider buffers whose other channels keep
  their bits;
* random data against fp64 on the rounded operands at the tolerance of
  tests/test_gpu_conv3_bf16_ops.py (atol 2e-6·√K·4, rtol 1e-5), the unrounded fp64 result as the
  negative control;
* reproducibility, equality with SCFLOW_CONV_BF16_3X3 for a plain launch, refusals.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import enc_bf16_restatement as er
from tests.test_gpu_gru_bf16_ops import close

pytestmark = pytest.mark.gpu

# (n, h, w, c0, cout): one workgroup, one stage; samples × row blocks, an odd number of 32-channel
# blocks, the neighbour-sample halo; four and eight column blocks; stage 2's and stage 3's shapes
SHAPES = [(1, 4, 32, 32, 1), (3, 12, 32, 64, 96), (1, 4, 128, 64, 64), (2, 8, 256, 64, 64),
          (2, 8, 64, 96, 96), (2, 32, 32, 128, 128)]
CASES = {"plain": (), "in_scale only": ("in",), "affine + ReLU": ("out", "relu"),
         "affine + res + ReLU": ("out", "res", "relu"), "all": ("in", "out", "res", "relu")}


@pytest.fixture(scope="module")
def ops():
    from scflow_amd import ops as _ops
    return _ops


def rows(x):  # NCHW → [pixels][channels]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def run(ops, d, pieces, strided=False, fmt=None):
    """One launch of the data ``d`` with the fused ``pieces``; returns the NCHW output on the CPU.
    ``strided``: source, output and residual are channel slices at offset 4 of wider NaN-filled
    buffers, and every bit outside the slices is checked afterwards."""
    from scflow_amd import _lib
    fmt = _lib.CONV_BF16_3X3N if fmt is None else fmt
    x, wt = d["x"], d["w"]
    n, c0, h, w = x.shape
    cout = wt.shape[0]
    M = n * h * w
    nan = float("nan")
    packed = ops.pack_conv_weight(wt.cuda(), c0, 0, w, 1, fmt)
    if strided:
        sbuf = torch.full((M, c0 + 8), nan, device="cuda")
        sbuf[:, 4:4 + c0] = rows(x).cuda()
        obuf = torch.full((M, cout + 7), nan, device="cuda")
        rbuf = torch.full((M, (cout + 3) // 4 * 4 + 8), nan, device="cuda")
        rbuf[:, 4:4 + cout] = rows(d["res"]).cuda()
        src, out, res = ops.Chan(sbuf, 4, c0), ops.Chan(obuf, 4, cout), ops.Chan(rbuf, 4, cout)
        before = [b.view(torch.int32).clone() for b in (sbuf, obuf, rbuf)]
    else:
        obuf = torch.full((M, cout), nan, device="cuda")
        src, out = ops.Chan.whole(rows(x).cuda()), ops.Chan.whole(obuf)
        rbuf = torch.zeros(M, (cout + 3) // 4 * 4, device="cuda")  # (sres is a multiple of 4 floats)
        rbuf[:, :cout] = rows(d["res"]).cuda()
        res = ops.Chan(rbuf, 0, cout)
    fused = {}
    if "in" in pieces:
        fused.update(in_scale=d["isc"].cuda(), in_shift=d["ish"].cuda())
    if "out" in pieces:
        fused.update(out_scale=d["osc"].cuda(), out_shift=d["osh"].cuda())
    if "res" in pieces:
        fused.update(res=res)
    ops.conv2d(src, packed, d["b"].cuda(), n, h, w, cout, 3, 3, 1, 1, "ReLU" if "relu" in pieces else None,
               out=out, bk=fmt, **fused)
    torch.cuda.synchronize()
    if strided:
        after = [b.view(torch.int32) for b in (sbuf, obuf, rbuf)]
        assert torch.equal(after[0], before[0]) and torch.equal(after[2], before[2])
        assert torch.equal(after[1][:, :4], before[1][:, :4])
        assert torch.equal(after[1][:, 4 + cout:], before[1][:, 4 + cout:])
    return ops.chan_to_nchw(out, n, h, w).cpu()


def restated(d, pieces, rounded=True):
    kw = {}
    if "in" in pieces:
        kw.update(in_scale=d["isc"], in_shift=d["ish"])
    if "out" in pieces:
        kw.update(out_scale=d["osc"], out_shift=d["osh"])
    if "res" in pieces:
        kw.update(res=d["res"])
    return er.launch(d["x"], d["w"], d["b"], act="ReLU" if "relu" in pieces else None, rounded=rounded, **kw)


# ------------------------------------------------------------------------------------ exact case
_exact = {}


def exact_data(n, h, w, c0, cout):
    key = (n, h, w, c0, cout)
    if key in _exact:
        return _exact[key]
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w + cout)
    pw2 = torch.tensor([0.5, 1.0, 2.0])
    x = torch.randint(-32, 33, (n, c0, h, w), generator=g).float()
    isc = pw2[torch.randint(0, 3, (n, c0), generator=g)]
    ish = torch.randint(-8, 9, (n, c0), generator=g).float()
    ish[:, ::3] = ish[:, ::3].abs() + 1  # positive shifts in every 32-channel block of every sample
    vals = torch.tensor([1.0, -1.0, 0.5, -0.5])
    wt = vals[torch.randint(0, 4, (cout, c0, 3, 3), generator=g)]
    wt = wt * (torch.rand(wt.shape, generator=g) < 0.08)
    # every (tap, 32-channel block) carries weights
    assert all(wt[:, 32 * b:32 * b + 32, ky, kx].abs().sum() > 0 or cout == 1
               for b in range(c0 // 32) for ky in range(3) for kx in range(3))
    assert wt.abs().sum() > 0
    d = dict(x=x, w=wt, isc=isc, ish=ish, b=torch.randint(-8, 9, (cout,), generator=g).float() / 4,
             osc=pw2[torch.randint(0, 3, (cout,), generator=g)],
             osh=torch.randint(-8, 9, (cout,), generator=g).float() / 4,
             res=torch.randint(-16, 17, (n, cout, h, w), generator=g).float())
    d["ref"] = {}
    for name, pieces in CASES.items():
        ref = restated(d, pieces)
        assert torch.equal(ref.float().double(), ref)  # exact in fp32
        xin = torch.relu(x * isc[:, :, None, None] + ish[:, :, None, None]) if "in" in pieces else x
        assert torch.equal(er.round_bf16(xin), xin)    # and the conv's input in bf16
        d["ref"][name] = ref.float()
    assert torch.equal(er.round_bf16(wt), wt)
    assert not torch.equal(d["ref"]["plain"], d["ref"]["in_scale only"])
    _exact[key] = d
    return d


@pytest.mark.parametrize("case", list(CASES), ids=[c.replace(" ", "_") for c in CASES])
@pytest.mark.parametrize("n,h,w,c0,cout", SHAPES)
def test_exact_case_is_bitwise(ops, n, h, w, c0, cout, case):
    d = exact_data(n, h, w, c0, cout)
    ref = d["ref"][case]
    for strided in (False, True):
        got = run(ops, d, CASES[case], strided)
        assert torch.equal(got, ref), \
            f"{case}, strided={strided}: {(got != ref).sum().item()} of {got.numel()} differ, " \
            f"first at {(got != ref).nonzero()[0].tolist()}"


def test_a_positive_shift_would_show_in_the_border():
    """The exact data separates "padding is 0" from "padding is relu(in_shift)" on the CPU alone:
    the restatement with the affine applied to a zero-padded input differs at the border."""
    d = exact_data(*SHAPES[1])
    x, isc, ish = d["x"], d["isc"][:, :, None, None], d["ish"][:, :, None, None]
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    wrong = torch.nn.functional.conv2d(torch.relu(xp * isc + ish).double(), d["w"].double(), d["b"].double())
    right = d["ref"]["in_scale only"].double()
    assert not torch.equal(wrong[:, :, 0], right[:, :, 0]) and not torch.equal(wrong[..., 0], right[..., 0])
    assert torch.equal(wrong[:, :, 1:-1, 1:-1], right[:, :, 1:-1, 1:-1])


# ------------------------------------------------------------------------------------ tolerance case
TOL_SHAPES = [(2, 8, 64, 96, 96), (2, 32, 32, 128, 128), (1, 4, 128, 64, 64)]
_random = {}


def random_data(n, h, w, c0, cout):
    key = (n, h, w, c0, cout)
    if key not in _random:
        g = torch.Generator().manual_seed(7 * c0 + w)
        d = dict(x=torch.randn(n, c0, h, w, generator=g),
                 w=torch.randn(cout, c0, 3, 3, generator=g) / np.sqrt(9 * c0),
                 b=torch.randn(cout, generator=g) * 0.1,
                 isc=torch.rand(n, c0, generator=g) + 0.5, ish=torch.randn(n, c0, generator=g) * 0.5,
                 osc=torch.rand(cout, generator=g) * 0.5 + 0.5,  # [0.5, 1]: the conv's error is not amplified
                 osh=torch.randn(cout, generator=g) * 0.2,
                 res=torch.randn(n, cout, h, w, generator=g))
        d["rounded"] = {c: restated(d, p) for c, p in CASES.items()}
        d["unrounded"] = {c: restated(d, p, rounded=False) for c, p in CASES.items()}
        _random[key] = d
    return _random[key]


def tolerance(c0):
    """tests/test_gpu_conv3_bf16_ops.py's: atol 2e-6·√K·4, rtol 1e-5, K = 9·c0."""
    return 2e-6 * np.sqrt(9 * c0) * 4, 1e-5


@pytest.mark.parametrize("case", list(CASES), ids=[c.replace(" ", "_") for c in CASES])
@pytest.mark.parametrize("n,h,w,c0,cout", TOL_SHAPES)
def test_random_data_within_the_direct_fp32_tolerance(ops, n, h, w, c0, cout, case):
    d = random_data(n, h, w, c0, cout)
    atol, rtol = tolerance(c0)
    got = run(ops, d, CASES[case], strided=True)
    ref = d["rounded"][case]
    close(got, ref, atol, rtol, f"enc conv3 ({n},{h},{w},{c0},{cout}) {case} (atol {atol:.2e})")
    if "relu" in CASES[case]:
        assert (ref == 0).any() and (ref > 0).any()


@pytest.mark.parametrize("case", ["in_scale only", "all"])
def test_negative_control_the_unrounded_result_is_outside_the_tolerance(ops, case):
    """The tolerance separates "rounded as specified" from "not rounded": on the CPU alone the two
    fp64 results are further apart than it allows, and so is the device from the unrounded one."""
    n, h, w, c0, cout = TOL_SHAPES[0]
    d = random_data(n, h, w, c0, cout)
    atol, rtol = tolerance(c0)
    un, rd = d["unrounded"][case], d["rounded"][case]
    print(f"{case}: rounded vs unrounded fp64 max |Δ| {(rd - un).abs().max().item():.3e} (atol {atol:.3e})")
    assert ((rd - un).abs() - (atol + rtol * un.abs())).max().item() > 0, \
        "the reference alone does not exceed the tolerance on this data"
    got = run(ops, d, CASES[case]).double()
    print(f"{case}: device vs unrounded fp64 max |Δ| {(got - un).abs().max().item():.3e}")
    assert ((got - un).abs() - (atol + rtol * un.abs())).max().item() > 0


# ------------------------------------------------------------------------------------ the rest
def test_two_runs_are_bitwise_equal(ops):
    d = random_data(*TOL_SHAPES[1])
    a, b = run(ops, d, CASES["all"], True), run(ops, d, CASES["all"], True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_a_plain_launch_equals_the_motion_encoder_formats(ops):
    from scflow_amd import _lib
    n, h, w, c0, cout = 2, 32, 32, 128, 64
    g = torch.Generator().manual_seed(11)
    d = dict(x=torch.randn(n, c0, h, w, generator=g), w=torch.randn(cout, c0, 3, 3, generator=g) / 34,
             b=torch.randn(cout, generator=g) * 0.1, res=torch.zeros(n, cout, h, w))
    for pieces in ((), ("relu",)):
        nine = run(ops, d, pieces, True)
        seven = run(ops, d, pieces, True, fmt=_lib.CONV_BF16_3X3)
        assert torch.equal(nine.view(torch.int32), seven.view(torch.int32))
    assert nine.abs().max() > 0


def test_refusals_leave_the_output_untouched(ops):
    """scflow_conv2d answers SCFLOW_EUNSUPPORTED (−2) outside the domain, SCFLOW_EALIGN (−3) for a
    misaligned stride and SCFLOW_EINVAL (−1) for half an affine before anything is launched: the
    output keeps its fill.  Through ``ops.conv2d`` the same calls raise ScflowError."""
    from scflow_amd import _lib
    from scflow_amd._lib import ScflowError
    n, h, w, c = 1, 8, 32, 64
    lib = _lib.load()
    out = torch.full((n * h * w, c), -5.0, device="cuda")
    src = torch.zeros(n * h * w, c, device="cuda")
    vec = torch.ones(n * c, device="cuda")
    packed = ops.pack_conv_weight(torch.zeros(c, c, 3, 3, device="cuda"), c, 0, w, 1, _lib.CONV_BF16_3X3N)

    def status(s=None, hh=h, ww=w, **over):
        a = ops.conv2d_args(ops.Chan.whole(src) if s is None else s, packed, None, n, hh, ww, c, 3, 3, 1, 1,
                            out=ops.Chan.whole(out), bk=_lib.CONV_BF16_3X3N)
        for k, v in over.items():
            setattr(a, k, v)
        return lib.scflow_conv2d(ctypes.byref(a), ops.raw_stream(0))
    assert status(stride=2) == -2
    assert status(ph=0, pw=0) == -2
    assert status(hh=6) == -2
    assert status(hh=16, ww=16) == -2
    assert status(hh=4, ww=48) == -2
    assert status(epilogue=_lib.EPI_GRU_Q, gate=out.data_ptr(), hid=out.data_ptr()) == -2
    assert status(bias_map=out.data_ptr(), sbm=c) == -2
    assert status(in_scale=vec.data_ptr()) == -1
    assert status(in_shift=vec.data_ptr()) == -1
    assert status(out_scale=vec.data_ptr()) == -1
    assert status(out_shift=vec.data_ptr()) == -1
    assert status(res=src.data_ptr(), sres=c + 2) == -3
    wide = torch.zeros(n * h * w, c + 2, device="cuda")
    assert status(ops.Chan(wide, 0, c)) == -3
    with pytest.raises(ScflowError):
        ops.conv2d(ops.Chan(wide, 0, c), packed, None, n, h, w, c, 3, 3, 1, 1, out=ops.Chan.whole(out),
                   bk=_lib.CONV_BF16_3X3N)
    with pytest.raises(ScflowError):
        ops.conv2d(ops.Chan.whole(src), packed, None, n, h, w, c, 3, 3, 1, 1, out=ops.Chan.whole(out),
                   bk=_lib.CONV_BF16_3X3N, in_scale=vec)
    with pytest.raises(ScflowError):  # a 16-wide map cannot even be packed
        ops.pack_conv_weight(torch.zeros(c, c, 3, 3, device="cuda"), c, 0, 16, 1, _lib.CONV_BF16_3X3N)
    torch.cuda.synchronize()
    assert (out == -5).all()
