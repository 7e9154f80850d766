"""The Winograd kernels' halo addressing and input affine at the shapes where they take another
path: two sources, a channel tail inside a stage of each, a single stage, image borders, n = 2.

F(4,5) (conv_wino5.h) and F(2×2,3×3) (conv_wino.h, and the pair launcher of conv_pair.h) form
their halo offsets once per source, blank the lanes of a source's missing channels in its last
stage, and carry the encoders' normalisation on load only in the instantiation a conv with
``in_scale`` launches.  Every case goes through ``ops.conv2d`` / ``ops.conv2d_pair`` and is held
against the fp64 direct conv under test_conv2d_variants' bound, |Δ| ≤ 8e-6·√K + 1e-5·|ref| with K =
input channels × taps.  The GRU epilogues' outputs are 1-Lipschitz functions of the conv (σ' ≤ ¼,
tanh' ≤ 1, the gate z in [0, 1] and h given), so the same bound holds for them.

The inputs are channel slices of wider buffers whose other columns hold NaN: a lane that reads a
channel its source does not have meets a zero weight, and NaN · 0 is still NaN.

The z|r epilogue takes an even number of output channels (scflow_conv2d refuses an odd one), so
its partial channel block is 34 channels where the other two epilogues run 33.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import switches

pytestmark = pytest.mark.gpu

FOREIGN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from scflow_amd import ops as o
    return o


def close(a, b, atol, rtol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    bad = ~(err <= atol + rtol * b.abs())  # a NaN is bad
    print(f"{what}: max err {err.max().item():.3e}, bound {atol:.3e} + {rtol:.0e}·|ref|")
    assert not bad.any(), f"{what}: max err {err.max().item():.3e} at {bad.nonzero()[0].tolist()}"


def bound(cin, taps):
    return 8e-6 * np.sqrt(cin * taps)


@lru_cache(maxsize=None)
def problem(n, h, w, c0, c1, cout, k, seed):
    """Inputs, the conv (kept on the CPU: runner_for launches a copy) and the fp64 conv with bias
    of one shape, computed once."""
    g = torch.Generator().manual_seed(seed)
    kh, kw = k
    x0 = torch.randn(n, c0, h, w, generator=g)
    x1 = torch.randn(n, c1, h, w, generator=g) if c1 else None
    conv = torch.nn.Conv2d(c0 + c1, cout, k, padding=(kh // 2, kw // 2))
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / np.sqrt(conv.weight[0].numel()))
        conv.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    xin = torch.cat([x0, x1], 1) if c1 else x0
    pre = F.conv2d(xin.double(), conv.weight.double(), conv.bias.double(), padding=(kh // 2, kw // 2))
    return x0, x1, conv, pre


def sliced(ops, x, off, extra):
    """NCHW x as the channel slice [off, off + c) of a NaN-filled [pixels, off + c + extra] buffer."""
    n, c, h, w = x.shape
    buf = torch.full((n * h * w, off + c + extra), FOREIGN, device="cuda")
    ops.nchw_into(x.cuda(), ops.Chan(buf, off, c))
    return ops.Chan(buf, off, c)


def runner_for(conv, act, shape):
    import copy
    from scflow_amd._lib import CONV_WINO
    from scflow_amd.modules import ConvRunner
    r = ConvRunner([copy.deepcopy(conv).cuda()], act)
    r._bk_shape, r._bk = shape, CONV_WINO
    return r


def nchw(ops, t, n, h, w):
    return ops.chan_to_nchw(ops.Chan.whole(t), n, h, w)


# ------------------------------------------------------------------------------ F(4,5)
@pytest.mark.parametrize("cout", [33, 64])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("w,c0,c1", [(32, 40, 24), (64, 32, 0)], ids=["two-sources-tails", "one-stage"])
@pytest.mark.parametrize("epi", ["plain", "zr", "q"])
@pytest.mark.parametrize("k", [(1, 5), (5, 1)], ids=["1x5", "5x1"])
def test_wino5_sources_and_tails(ops, k, epi, w, c0, c1, n, cout):
    from scflow_amd import _lib
    h = 8
    if epi == "zr":
        cout += cout & 1
    x0, x1, conv, pre = problem(n, h, w, c0, c1, cout, k, 3)
    M = n * h * w
    s0 = sliced(ops, x0, 4, 4)
    s1 = sliced(ops, x1, 8, 4) if c1 else None
    r = runner_for(conv, None, (n, h, w, c0, c1))
    atol, what = bound(c0 + c1, 5), f"F(4,5) {k} {epi} n={n} w={w} {c0}+{c1}->{cout}"
    g = torch.Generator().manual_seed(5)
    if epi == "plain":
        out = torch.full((M, cout + 3), -5.0, device="cuda")
        r.run(s0, ops.Chan(out, 3, cout), n, h, w, src1=s1)
        assert ops.conv_plan_kind(r.args(s0, ops.Chan(out, 3, cout), n, h, w, src1=s1)) == _lib.PLAN_WINO5
        assert (out[:, :3] == -5).all()
        close(ops.chan_to_nchw(ops.Chan(out, 3, cout), n, h, w), pre, atol, 1e-5, what)
    elif epi == "zr":
        hc = cout // 2
        hid = torch.tanh(torch.randn(M, hc, generator=g))
        gate = torch.full((M, hc), -5.0, device="cuda")
        rh = torch.full((M, hc), -5.0, device="cuda")
        kw = dict(src1=s1, epilogue=_lib.EPI_GRU_ZR, gate=ops.Chan.whole(gate), rh=ops.Chan.whole(rh),
                  hid=ops.Chan.whole(hid.cuda()))
        assert ops.conv_plan_kind(r.args(s0, None, n, h, w, **kw)) == _lib.PLAN_WINO5
        r.run(s0, None, n, h, w, **kw)
        hn = hid.view(n, h, w, hc).permute(0, 3, 1, 2).double()
        close(nchw(ops, gate, n, h, w), torch.sigmoid(pre[:, :hc]), atol, 1e-5, what + " z")
        close(nchw(ops, rh, n, h, w), torch.sigmoid(pre[:, hc:]) * hn, atol, 1e-5, what + " r·h")
    else:
        hid = torch.tanh(torch.randn(M, cout, generator=g))
        z = torch.rand(M, cout, generator=g)
        dh = hid.cuda()
        kw = dict(src1=s1, epilogue=_lib.EPI_GRU_Q, gate=ops.Chan.whole(z.cuda()), hid=ops.Chan.whole(dh))
        assert ops.conv_plan_kind(r.args(s0, None, n, h, w, **kw)) == _lib.PLAN_WINO5
        r.run(s0, None, n, h, w, **kw)

        def to(t):
            return t.view(n, h, w, cout).permute(0, 3, 1, 2).double()
        close(nchw(ops, dh, n, h, w), (1 - to(z)) * to(hid) + to(z) * torch.tanh(pre), atol, 1e-5,
              what + " h")


# ------------------------------------------------------------------------------ F(2×2,3×3)
def affine(n, c, seed):
    """Per (image, channel) scale and a positive shift: relu(0·scale + shift) > 0, so padding that
    went through the affine would show at every border."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, c, generator=g) + 0.5, torch.rand(n, c, generator=g) + 0.5


def wino_ref(pre_problem, isc, ish):
    """fp64 conv of relu(x·scale + shift), zero padding applied after the affine."""
    x0, _, conv, _ = pre_problem
    xa = torch.relu(x0.double() * isc.double()[:, :, None, None] + ish.double()[:, :, None, None])
    return F.conv2d(xa, conv.weight.double(), conv.bias.double(), padding=1)


def wino_args(ops, prob, n, h, w, cout, out, aff=None):
    """scflow_conv_args of the F(2×2,3×3) launch of ``prob`` into the [pixels, cout + 3] ``out``."""
    from scflow_amd import _lib
    x0, x1, conv, _ = prob
    c0, c1 = x0.shape[1], 0 if x1 is None else x1.shape[1]
    r = runner_for(conv, None, (n, h, w, c0, c1))
    packed, bias = r.packed(c0, c1, w, _lib.CONV_WINO)
    fused = {} if aff is None else dict(in_scale=aff[0].cuda(), in_shift=aff[1].cuda())
    s0, s1 = sliced(ops, x0, 4, 4), sliced(ops, x1, 8, 4) if c1 else None
    a = ops.conv2d_args(s0, packed, bias, n, h, w, cout, 3, 3, 1, 1, None, out=ops.Chan(out, 3, cout),
                        src1=s1, bk=_lib.CONV_WINO, **fused)
    a._keep += (s0, s1) + tuple(fused.values())  # the struct outlives this call: so must its inputs
    assert ops.conv_plan_kind(a) == _lib.PLAN_WINO
    return a


@pytest.mark.parametrize("nbw", [0, 2], ids=["nbw-picked", "nbw2"])
@pytest.mark.parametrize("cout", [30, 64, 96])
@pytest.mark.parametrize("w", [32, 64])
def test_wino_sources_and_tails(ops, w, cout, nbw, monkeypatch):
    """Two sources with a channel tail in a stage of each (40 + 24), n = 1: 32 and 64 output
    channels per workgroup."""
    n, h = 1, 8
    prob = problem(n, h, w, 40, 24, cout, (3, 3), 7)
    out = torch.full((n * h * w, cout + 3), -5.0, device="cuda")
    with switches(monkeypatch, SCFLOW_WINO_NBW=nbw):
        a = wino_args(ops, prob, n, h, w, cout, out)
        ops.conv2d_launch(a, out)
    assert (out[:, :3] == -5).all()
    close(ops.chan_to_nchw(ops.Chan(out, 3, cout), n, h, w), prob[3], bound(64, 9), 1e-5,
          f"F(2x2,3x3) w={w} 40+24->{cout} nbw={nbw}")


@pytest.mark.parametrize("nbw", [0, 2], ids=["nbw-picked", "nbw2"])
@pytest.mark.parametrize("cout", [30, 64, 96])
@pytest.mark.parametrize("n,w", [(1, 32), (1, 64), (2, 32), (2, 64)])
def test_wino_input_affine(ops, n, w, cout, nbw, monkeypatch):
    """The affine instantiation (one source of 40 channels: a tail of 8 in the second stage), per
    image scales at n = 2, and the same conv without the affine beside it; the zero padding stays
    zero at the image borders (8 rows: both row blocks of an image touch one)."""
    h = 8
    prob = problem(n, h, w, 40, 0, cout, (3, 3), 9)
    aff = affine(n, 40, 13)
    for use, ref in ((aff, wino_ref(prob, *aff)), (None, prob[3])):
        out = torch.full((n * h * w, cout + 3), -5.0, device="cuda")
        with switches(monkeypatch, SCFLOW_WINO_NBW=nbw):
            ops.conv2d_launch(wino_args(ops, prob, n, h, w, cout, out, use), out)
        assert (out[:, :3] == -5).all()
        close(ops.chan_to_nchw(ops.Chan(out, 3, cout), n, h, w), ref, bound(40, 9), 1e-5,
              f"F(2x2,3x3) n={n} w={w} 40->{cout} nbw={nbw} affine={use is not None}")


@pytest.mark.parametrize("couts", [(30, 64), (96, 30), (64, 64)])
@pytest.mark.parametrize("w", [32, 64])
def test_wino_pair(ops, w, couts):
    """scflow_conv2d_pair on two F(2×2,3×3) convs: the grouped kernel for two plain convs (two
    sources with tails each), and two launches once a half brings the input affine — which the
    grouped kernel's bodies do not carry — with the same results either way."""
    from scflow_amd import _lib
    n, h = 1, 8
    ca, cb = couts
    pa, pb = problem(n, h, w, 40, 24, ca, (3, 3), 21), problem(n, h, w, 40, 24, cb, (3, 3), 22)
    oa = torch.full((n * h * w, ca + 3), -5.0, device="cuda")
    ob = torch.full((n * h * w, cb + 3), -5.0, device="cuda")
    aa, ab = wino_args(ops, pa, n, h, w, ca, oa), wino_args(ops, pb, n, h, w, cb, ob)
    assert ops.conv_plan_kind(aa, ab) == _lib.PAIR_WINO
    ops.conv2d_pair(aa, ab, oa)
    close(ops.chan_to_nchw(ops.Chan(oa, 3, ca), n, h, w), pa[3], bound(64, 9), 1e-5, f"pair a w={w} {couts}")
    close(ops.chan_to_nchw(ops.Chan(ob, 3, cb), n, h, w), pb[3], bound(64, 9), 1e-5, f"pair b w={w} {couts}")
    # an affine half (one source): two launches, each its own instantiation
    pc = problem(n, h, w, 40, 0, ca, (3, 3), 23)
    aff = affine(n, 40, 24)
    oc = torch.full((n * h * w, ca + 3), -5.0, device="cuda")
    ob.fill_(-5.0)
    ac = wino_args(ops, pc, n, h, w, ca, oc, aff)
    assert ops.conv_plan_kind(ac, ab) == _lib.PAIR_NONE
    ops.conv2d_pair(ac, ab, oc)
    close(ops.chan_to_nchw(ops.Chan(oc, 3, ca), n, h, w), wino_ref(pc, *aff), bound(40, 9), 1e-5,
          f"pair affine half w={w} {couts}")
    close(ops.chan_to_nchw(ops.Chan(ob, 3, cb), n, h, w), pb[3], bound(64, 9), 1e-5,
          f"pair plain half w={w} {couts}")


@pytest.mark.parametrize("k", [(3, 3), (1, 5), (5, 1)], ids=["3x3", "1x5", "5x1"])
def test_cut_loop_long_pieces(ops, k):
    """104 + 72 channels: three whole stages before source 0's tail of 8, then two whole stages of
    source 1 and its tail of 8 (7 stages) — every piece of the cut stage loop but the last runs
    more than one iteration, and the next change lies up to three stages ahead."""
    from scflow_amd import _lib
    n, h, w, c0, c1, cout = 1, 8, 32, 104, 72, 64
    x0, x1, conv, pre = problem(n, h, w, c0, c1, cout, k, 31)
    s0, s1 = sliced(ops, x0, 4, 4), sliced(ops, x1, 8, 4)
    r = runner_for(conv, None, (n, h, w, c0, c1))
    out = torch.full((n * h * w, cout + 3), -5.0, device="cuda")
    a = r.args(s0, ops.Chan(out, 3, cout), n, h, w, src1=s1)
    assert ops.conv_plan_kind(a) == (_lib.PLAN_WINO if k == (3, 3) else _lib.PLAN_WINO5)
    ops.conv2d_launch(a, out)
    assert (out[:, :3] == -5).all()
    close(ops.chan_to_nchw(ops.Chan(out, 3, cout), n, h, w), pre, bound(c0 + c1, k[0] * k[1]), 1e-5,
          f"{k} {c0}+{c1}->{cout}")
