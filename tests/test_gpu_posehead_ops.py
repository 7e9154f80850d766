"""GPU: every launch of the pose head (MultiClassPoseHead, scflow_amd/csrc/posehead.hip and the
MFMA conv's two-source / K-split / norm-on-load form in encoder.hip) on its own against the fp64
restatement (tests/posehead_restatement.py, pinned to the oracle by tests/test_posehead_host.py),
at the shapes where the tile, slab and row-block logic can go wrong: batch 1, ragged pixel tiles,
uneven and single-unit K slabs, slabs that lie in the second source, every slab-count template of
the GroupNorm reduce and both of its channel-block forms, FC row blocks past 32 rows.

Inputs are channel slices of wider buffers (offsets multiples of 4) filled with a foreign value
around the slice; outputs sit inside sentinel-filled buffers and nothing outside the written range
may change.  Shapes, seeds and tolerances: tests/posehead_cases.py (its docstring derives them;
the GroupNorm bound's measured part is recorded there).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import posehead_cases as pc
from tests import posehead_restatement as rs
from tests.helpers import switches

pytestmark = pytest.mark.gpu

SENT = pc.SENTINEL


@pytest.fixture(scope="module")
def ops():
    from scflow_amd import ops as o
    return o


def close(a, b, atol, rtol=0.0, what=""):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    bad = (err > lim)
    assert not bad.any(), f"{what}: max err {err.max().item():.3e} at {bad.nonzero()[0].tolist()}"


def within(got, ref, bound, what):
    """|got − ref| ≤ bound elementwise, in fp64."""
    err = (got.detach().cpu().double() - ref).abs()
    bad = err > bound
    assert not bad.any(), (f"{what}: err {err[bad].max().item():.3e} over its bound at "
                           f"{bad.nonzero()[0].tolist()} (max err {err.max().item():.3e})")


def dev(x):
    return None if x is None else x.cuda()


class Guarded:
    """An output tensor inside a sentinel-filled buffer: ``check`` asserts that the launch wrote
    every element of the range it owns and nothing else."""

    def __init__(self, *shape, pad=64):
        numel = int(np.prod(shape))
        self.buf = torch.full((numel + 2 * pad,), SENT, device="cuda")
        self.pad = pad
        self.t = self.buf[pad:pad + numel].view(*shape)

    def check(self, what, cols=None):
        torch.cuda.synchronize()
        assert (self.buf[:self.pad] == SENT).all() and (self.buf[-self.pad:] == SENT).all(), \
            f"{what}: wrote outside its output"
        own = self.t if cols is None else self.t[..., :cols]
        assert not (own == SENT).any(), f"{what}: left part of its output unwritten"
        if cols is not None:
            assert (self.t[..., cols:] == SENT).all(), f"{what}: wrote past its channels"
        return own.cpu().double()


def chan(ops, x_nchw, off, extra):
    """x as channels [off, off + c) of a wider channels-last buffer filled with a foreign value."""
    n, c, h, w = x_nchw.shape
    buf = torch.full((n * h * w, off + c + extra), 9.0, device="cuda")
    ops.nchw_into(x_nchw.contiguous().cuda(), ops.Chan(buf, off, c))
    return ops.Chan(buf, off, c)


def nchw(slabs, ksplit, n, oh, ow, cout):
    """[ksplit·n·oh·ow, cout] channels-last slabs → [ksplit, n, cout, oh, ow]."""
    return slabs.view(ksplit, n, oh, ow, cout).permute(0, 1, 4, 2, 3)


# ------------------------------------------------------------------------------ (a) gather conv
@pytest.mark.parametrize("case", [c for c, _ in pc.GATHER_CASES], ids=[i for _, i in pc.GATHER_CASES])
def test_ph_conv_gather(ops, case):
    """scflow_ph_conv_split against conv / conv_slab_chunks: every slab and the slab sum.  M < 32
    (batch 1's conv3: half a pixel tile), M % 32 ≠ 0 (48, 80), K chunks split unevenly and inside
    a tap, one chunk per slice, two sources with cin padded to 32, cout 33 / 40 / 8.  With norm the
    shift is positive on half the channels: a border pixel off by O(0.1) is norm-on-load applied
    to the zero padding (test_posehead_host.py::test_padding_check_has_teeth)."""
    n, h, w, c0, c1, cout, k, stride, pad, ksplit, norm, bias = case
    d = pc.gather_inputs(case)
    src0 = chan(ops, d["x"][:, :c0], 4, 4)
    src1 = chan(ops, d["x"][:, c0:], 8, 4) if c1 else None
    packed = ops.ph_conv_pack(d["w"].cuda())
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    out = Guarded(ksplit * n * oh * ow, cout)
    ops.ph_conv(src0, src1, packed, dev(d["bias"]), n, h, w, cout, k, stride, pad, out.t,
                dev(d["scale"]), dev(d["shift"]), ksplit=ksplit)
    got = nchw(out.check(f"ph_conv {case}"), ksplit, n, oh, ow, cout)
    cin = c0 + c1
    bounds = rs.split_bounds(rs.chunk_count(cin, k, k), ksplit)
    bref = 0 if d["bias"] is None else d["bias"].double()[None, :, None, None]
    for z, (lo, hi) in enumerate(bounds):
        ref = rs.conv_slab_chunks(d["x"], d["w"], stride, pad, d["scale"], d["shift"], lo, hi) + bref
        close(got[z], ref, *pc.conv_tol(rs.chunk_real_k(cin, k, k, lo, hi)),
              f"ph_conv {case} slab {z} (chunks {lo}..{hi})")
    whole = rs.conv(d["x"], d["w"], d["bias"], stride, pad, d["scale"], d["shift"])
    close(got.sum(0), whole, *pc.conv_tol(cin * k * k), f"ph_conv {case} slab sum")


def test_ph_conv_split_with_bias_raises(ops):
    from scflow_amd._lib import ScflowError
    d = pc.conv_inputs(1, 1, 5, 5, 16, 8, 3, norm=False, bias=True)
    src = chan(ops, d["x"], 4, 4)
    out = Guarded(3 * 25, 8)
    with pytest.raises(ScflowError):
        ops.ph_conv(src, None, ops.ph_conv_pack(d["w"].cuda()), d["bias"].cuda(), 1, 5, 5, 8, 3, 1, 1,
                    out.t, ksplit=3)
    torch.cuda.synchronize()
    assert (out.buf == SENT).all()


# ------------------------------------------------------------------------------ (b) MFMA conv
@pytest.mark.parametrize("case", [c for c, _ in pc.ENC_CASES], ids=[i for _, i in pc.ENC_CASES])
def test_enc_conv_posehead_form(ops, case):
    """scflow_enc_conv with src1 / ksplit / in_scale (the pose head's conv1 and conv2) against
    conv / conv_slab: every slab and the slab sum.  14 stages over 14 (one stage per slice) and
    over 5 (uneven), a last slab that lies entirely in src1, the per-image scale table indexed by
    the concatenated channel across the source boundary, cout 80 (not a multiple of 64), the
    stride-1 tile, and ksplit = 1 with bias + ReLU.  Norm-on-load next to the zero padding as in
    test_ph_conv_gather."""
    n, h, w, cin, cin1, cout, stride, ksplit, norm = case
    d = pc.enc_inputs(case)
    src0 = chan(ops, d["x"][:, :cin], 4, 4)
    src1 = chan(ops, d["x"][:, cin:], 8, 4) if cin1 else None
    packed = ops.enc_conv_pack(d["w"].cuda())
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    out = Guarded(ksplit * n * oh * ow, cout + 4)
    ops.enc_conv(src0, packed, dev(d["bias"]), n, h, w, cin, cout, 3, stride, 1, out.t,
                 in_scale=dev(d["scale"]), in_shift=dev(d["shift"]),
                 act="ReLU" if ksplit == 1 else None, src1=src1, ksplit=ksplit)
    got = nchw(out.check(f"enc_conv {case}", cols=cout).contiguous(), ksplit, n, oh, ow, cout)
    ctot = cin + cin1
    whole = rs.conv(d["x"], d["w"], d["bias"], stride, 1, d["scale"], d["shift"])
    if ksplit == 1:
        close(got[0], torch.relu(whole), *pc.conv_tol(ctot * 9), f"enc_conv {case}")
        return
    bounds = rs.split_bounds(ctot // 16, ksplit)
    if "all-src1" in dict(pc.ENC_CASES)[case]:
        assert 16 * bounds[-1][0] >= cin  # the last slab reads src1 only
    for z, (lo, hi) in enumerate(bounds):
        ref = rs.conv_slab(d["x"], d["w"], stride, 1, d["scale"], d["shift"], 16 * lo, 16 * hi)
        close(got[z], ref, *pc.conv_tol((hi - lo) * 16 * 9),
              f"enc_conv {case} slab {z} (stages {lo}..{hi})")
    close(got.sum(0), whole, *pc.conv_tol(ctot * 9), f"enc_conv {case} slab sum")


def test_enc_conv_split_with_bias_raises(ops):
    from scflow_amd._lib import ScflowError
    d = pc.conv_inputs(2, 1, 16, 16, 32, 64, 3, norm=False, bias=True)
    src = chan(ops, d["x"], 4, 4)
    out = Guarded(2 * 64, 64)
    with pytest.raises(ScflowError):
        ops.enc_conv(src, ops.enc_conv_pack(d["w"].cuda()), d["bias"].cuda(), 1, 16, 16, 32, 64, 3,
                     2, 1, out.t, ksplit=2)
    torch.cuda.synchronize()
    assert (out.buf == SENT).all()


# ------------------------------------------------------------------------------ (c) GroupNorm
def _gn_case(ops, case):
    ns, hw, c, groups = case
    n = pc.GN_N
    parts, gamma, beta = pc.gn_inputs(case)
    y_ref, ybound, (sc_ref, sh_ref) = pc.gn_reference(case)
    tol_sc, tol_sh = pc.gn_tolerances(case)
    pd = parts.view(ns, n * hw, c).cuda()
    launches = [("reduce", Guarded(n * hw, c))] + ([("stats", None)] if ns == 1 else [])
    for form, y in launches:
        scale, shift = Guarded(n, c), Guarded(n, c)
        if form == "reduce":
            ops.ph_gn_reduce(pd, ns, y.t, n, hw, c, groups, gamma.cuda(), beta.cuda(), pc.GN_EPS,
                             scale.t, shift.t)
            yk = y.check(f"gn_{form} {case} y")
            within(yk.view(n, hw, c), y_ref, ybound, f"gn_reduce {case} slab sum")
        else:
            ops.ph_gn_stats(pd[0], n, hw, c, groups, gamma.cuda(), beta.cuda(), pc.GN_EPS, scale.t,
                            shift.t)
            yk = parts[0].double().view(n * hw, c)
        sc = scale.check(f"gn_{form} {case} scale")
        sh = shift.check(f"gn_{form} {case} shift")
        within(sc, sc_ref, tol_sc, f"gn_{form} {case} scale")
        within(sh, sh_ref, tol_sh, f"gn_{form} {case} shift")
        # what the next layer computes from them, in fp32, against fp64 GroupNorm + ReLU
        act = torch.relu(yk.float().view(n, hw, c) * sc.float()[:, None, :] + sh.float()[:, None, :])
        ref = torch.relu(F.group_norm(y_ref.permute(0, 2, 1), groups, gamma.double(), beta.double(),
                                      pc.GN_EPS)).permute(0, 2, 1)
        close(act, ref, 1e-5, 1e-5, f"gn_{form} {case} relu(y·scale + shift)")


@pytest.mark.parametrize("case", pc.GN_CASES,
                         ids=lambda c: "ns{}-hw{}-c{}-g{}".format(*c))
def test_ph_gn_reduce(ops, case):
    """scflow_ph_gn_reduce (and scflow_ph_gn_stats at one slab) against gn_affine of the fp64 slab
    sum.  Slab counts 1, 2, 3, 4, 8 (compile-time templates; 1 and 3 run nowhere else) and 5, 14
    (generic loop; 14 is batch 1's conv1), each at hw = 16 (tail loop only, most pixel slots idle)
    and hw = 300 (an unrolled round plus a ragged tail); hw = 256 (exactly one unrolled round) and
    37 (ragged tail only); 16-channel blocks (group sizes 4, 16, 1) and the 32-channel block form
    that 32-channel groups force (c = 64, groups = 2)."""
    _gn_case(ops, case)


@pytest.mark.parametrize("case", pc.GN_CB32_CASES, ids=lambda c: "ns{}-hw{}-c{}-g{}".format(*c))
def test_ph_gn_reduce_cb32_switch(ops, case, monkeypatch):
    """The 32-channel block form chosen by SCFLOW_GNR_CB=32 at the pose head's group shape."""
    with switches(monkeypatch, SCFLOW_GNR_CB=32):
        _gn_case(ops, case)


def test_ph_gn_reduce_unsupported_channels_raises(ops):
    from scflow_amd._lib import ScflowError
    x = torch.randn(2, 3 * 16, 48).cuda()
    y, sc, sh = Guarded(3 * 16, 48), Guarded(3, 48), Guarded(3, 48)
    with pytest.raises(ScflowError):  # c = 48 is no multiple of 32
        ops.ph_gn_reduce(x, 2, y.t, 3, 16, 48, 3, torch.ones(48).cuda(), torch.zeros(48).cuda(),
                         1e-5, sc.t, sh.t)
    torch.cuda.synchronize()
    assert all((t.buf == SENT).all() for t in (y, sc, sh))


# ------------------------------------------------------------------------------ (d) FCs
def wide(x, off=4, extra=4):
    """x [m, k] as columns [off, off + k) of a wider buffer → (view, ldx)."""
    m, k = x.shape
    buf = torch.full((m, off + k + extra), 9.0, device="cuda")
    buf[:, off:off + k] = x.cuda()
    return buf[:, off:off + k], off + k + extra


@pytest.mark.parametrize("k,n", [(16, 5), (272, 40), (2048, 256)])
@pytest.mark.parametrize("m", [1, 16, 17, 32, 33, 50])
def test_ph_fc_plain(ops, m, k, n):
    """scflow_ph_fc on a plain input: one row tile (m ≤ 16), two (17, 32), and the row-block loop
    with its re-parking barrier at m > 32 (33: a one-row last block; 50), with and without ReLU
    and bias."""
    x, W, b = pc.fc_inputs(100 + m + k, m, k, n)
    xv, ldx = wide(x)
    for relu in (True, False):
        for bias in (b, None):
            y = Guarded(m, n)
            ops.ph_fc(xv, ldx, m, k, W.cuda(), dev(bias), y.t, n, relu)
            got = y.check(f"ph_fc m{m} k{k} n{n}")
            close(got, rs.fc(x, W, bias, relu), *pc.conv_tol(k),
                  f"ph_fc m{m} k{k} n{n} relu={relu} bias={bias is not None}")


@pytest.mark.parametrize("m", [3, 33])
def test_ph_fc_from_conv_output(ops, m):
    """scflow_ph_fc in gn_c mode (the unsplit FC1, the path of more than 32 samples): a raw conv
    output [m][16][128] normalised on load, the weight through scflow_ph_fc_permute, against
    fc_from_conv with the NCHW-order weight."""
    g = torch.Generator().manual_seed(200 + m)
    y = torch.randn(m, 16, 128, generator=g)
    scale = 0.5 * torch.randn(m, 128, generator=g) + 1.0
    shift = 0.5 * torch.randn(m, 128, generator=g)
    _, W, b = pc.fc_inputs(201 + m, 1, 2048, 40)
    Wp = ops.ph_fc_permute(W.cuda(), 128, 16)
    out = Guarded(m, 40)
    ops.ph_fc(y.cuda().view(m, 2048), 2048, m, 2048, Wp, b.cuda(), out.t, 40, True, gn_c=128,
              scale=scale.cuda(), shift=shift.cuda())
    close(out.check(f"ph_fc gn_c m{m}"), rs.fc_from_conv(y, scale, shift, W, b, True),
          *pc.conv_tol(2048), f"ph_fc gn_c m{m}")


@pytest.mark.parametrize("n,c,hw", [(7, 128, 16), (5, 12, 5)])
def test_ph_fc_permute(ops, n, c, hw):
    """A copy: exact."""
    W = torch.randn(n, c * hw, generator=torch.Generator().manual_seed(c))
    assert torch.equal(ops.ph_fc_permute(W.cuda(), c, hw).cpu(), rs.fc_permute(W, c, hw))


@pytest.mark.parametrize("k,n,ksplit", [(272, 40, 4), (272, 40, 17), (2048, 256, 4)])
@pytest.mark.parametrize("m", [1, 5, 32])
def test_ph_fc_split(ops, m, k, n, ksplit):
    """scflow_ph_fc_split: every partial slab and their sum.  17 K groups over 4 slices (uneven)
    and over 17 (one group per slice)."""
    x, W, _ = pc.fc_inputs(300 + m + k + ksplit, m, k, n)
    xv, ldx = wide(x)
    parts = Guarded(ksplit, m, n)
    ops.ph_fc_split(xv, ldx, m, k, W.cuda(), parts.t, n, ksplit)
    got = parts.check(f"ph_fc_split m{m} k{k} ks{ksplit}")
    for z, (lo, hi) in enumerate(rs.split_bounds(k // 16, ksplit)):
        sl = slice(16 * lo, 16 * hi)
        close(got[z], rs.fc(x[:, sl], W[:, sl], None, False), *pc.conv_tol(16 * (hi - lo)),
              f"ph_fc_split m{m} k{k} slab {z} of {ksplit}")
    close(got.sum(0), rs.fc(x, W, None, False), *pc.conv_tol(k), f"ph_fc_split m{m} k{k} sum")


def test_ph_fc_split_over_32_rows_raises(ops):
    from scflow_amd._lib import ScflowError
    x, W, _ = pc.fc_inputs(5, 33, 272, 40)
    parts = Guarded(4, 33, 40)
    with pytest.raises(ScflowError):
        ops.ph_fc_split(x.cuda(), 272, 33, 272, W.cuda(), parts.t, 40, 4)
    torch.cuda.synchronize()
    assert (parts.buf == SENT).all()


@pytest.mark.parametrize("m", [1, 5, 32])
def test_ph_fc_split_chain(ops, m):
    """FC1 (split) → FC2 reading FC1's partial sums (xsplit, xbias): FC2's slabs against
    fc_from_partials of the partial sums FC1 wrote, and the chain's sum against the two layers in
    fp64."""
    x, W1, b1 = pc.fc_inputs(400 + m, m, 272, 64)
    _, W2, b2 = pc.fc_inputs(401 + m, 1, 64, 24)
    p1, p2 = Guarded(4, m, 64), Guarded(2, m, 24)
    ops.ph_fc_split(x.cuda(), 272, m, 272, W1.cuda(), p1.t, 64, 4)
    ops.ph_fc_split(p1.t, 64, m, 64, W2.cuda(), p2.t, 24, 2, xsplit=4, xbias=b1.cuda())
    g1, g2 = p1.check(f"fc chain m{m} FC1"), p2.check(f"fc chain m{m} FC2")
    for z, (lo, hi) in enumerate(rs.split_bounds(4, 2)):
        sl = slice(16 * lo, 16 * hi)
        ref = rs.fc(rs.from_partials(g1, b1)[:, sl], W2[:, sl], None, False)
        close(g2[z], ref, *pc.conv_tol(32), f"fc chain m{m} FC2 slab {z}")
    ref = rs.fc(rs.fc(x, W1, b1, True), W2, b2, True)
    close(rs.from_partials(g2, b2), ref, *pc.conv_tol(272), f"fc chain m{m}")


@pytest.mark.parametrize("m", [3, 20])
def test_ph_fc_sum(ops, m):
    """scflow_ph_fc_sum (an exported entry without a caller in the modules): the unsplit FC on a
    split producer's partial sums, one and two row tiles."""
    g = torch.Generator().manual_seed(500 + m)
    parts = torch.randn(4, m, 64, generator=g)
    xb = 0.1 * torch.randn(64, generator=g)
    _, W, b = pc.fc_inputs(501 + m, 1, 64, 24)
    for relu in (True, False):
        for bias in (b, None):
            y = Guarded(m, 24)
            ops.ph_fc_sum(parts.cuda(), 4, m, 64, xb.cuda(), W.cuda(), dev(bias), y.t, 24, relu)
            close(y.check(f"ph_fc_sum m{m}"), rs.fc_from_partials(parts, xb, W, bias, relu),
                  *pc.conv_tol(64), f"ph_fc_sum m{m} relu={relu} bias={bias is not None}")


@pytest.mark.parametrize("xsplit", [0, 4], ids=["plain", "xsplit4"])
@pytest.mark.parametrize("rch", [6, 4])
@pytest.mark.parametrize("m", [1, 3, 33])
def test_ph_heads(ops, m, rch, xsplit):
    """scflow_ph_heads / scflow_ph_heads_sum: label = [7, 3, 12, …] and every row uses class 7
    (test_posehead_host.py::test_label0_check_has_teeth: a row's own label fails this)."""
    x, xb, Wr, br, Wt, bt, label = pc.heads_inputs(600 + m + rch + xsplit, m, 256, rch, xsplit=xsplit)
    drot, dt = Guarded(m, rch), Guarded(m, 3)
    ops.ph_heads(x.cuda(), m, 256, Wr.cuda(), br.cuda(), rch, Wt.cuda(), bt.cuda(), label.cuda(), 21,
                 drot.t, dt.t, xsplit=xsplit, xbias=xb.cuda() if xsplit else None)
    xin = rs.from_partials(x, xb) if xsplit else x
    r_ref, t_ref = rs.heads(xin, Wr, br, Wt, bt, label, rch)
    np.testing.assert_allclose(drot.check(f"ph_heads m{m} drot").numpy(), r_ref.numpy(), rtol=1e-5,
                               atol=1e-6)
    np.testing.assert_allclose(dt.check(f"ph_heads m{m} dt").numpy(), t_ref.numpy(), rtol=1e-5,
                               atol=1e-6)
