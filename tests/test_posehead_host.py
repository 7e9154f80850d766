"""CPU: the fp64 restatement of the pose head's launches (tests/posehead_restatement.py) pinned to
the oracle, and proof that the GPU comparisons built on it (tests/test_gpu_posehead_ops.py) have
teeth: the errors those tests are there to catch — the input affine applied to the zero padding, a
K-slab boundary off by one chunk / stage, each row using its own label — move the restatement by
far more than the tolerances the GPU tests use, at the shapes they use."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import posehead_cases as pc
from tests import posehead_restatement as rs

orc = pytest.importorskip("oracle.scflow_oracle")


def exceeds(a, b, atol, rtol):
    """Whether a vs the reference b fails the GPU tests' close(atol, rtol) somewhere."""
    return bool(((a - b).abs() > atol + rtol * b.abs()).any())


def affine_on_padding(x, w, stride, pad, scale, shift):
    """The bug the padding checks are for: pad first, then relu(x·scale + shift) everywhere, so
    the padding becomes relu(shift)."""
    xp = F.pad(x.double(), (pad, pad, pad, pad))
    return F.conv2d(rs.norm_on_load(xp, scale, shift), w.double(), None, stride=stride)


def border_mask(oh, ow):
    m = torch.zeros(oh, ow, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def test_restatement_composes_to_the_oracle_head():
    """conv → gn_affine → conv(norm on load) ×3 → fc_from_conv → fc → heads, against
    oracle.scflow_oracle.pose_head (itself pinned to the reference) within 1e-10."""
    from scflow_amd import synthetic
    from scflow_amd.modules import MultiClassPoseHead
    n, feat = 2, 32
    head = MultiClassPoseHead(21, 224, "Basic", dict(type="GN", num_groups=32), dict(type="ReLU"),
                              feat_size=(feat, feat), rotation_mode="ortho6d")
    synthetic.fill_module_(head, seed=7)
    g = torch.Generator().manual_seed(8)
    x = torch.relu(torch.randn(n, 224, feat, feat, generator=g)).double()
    label = torch.randint(0, 21, (n,), generator=g)
    sd = {f"pose_pred.{k}": v.double() for k, v in head.state_dict().items()}
    r_ref, t_ref = orc.pose_head(sd, x, label, 21)
    p = {k: v.double() for k, v in head.state_dict().items()}
    scale = shift = None
    y = x
    for i in range(3):
        y = rs.conv(y, p[f"conv_layers.{i}.conv.weight"], None, 2, 1, scale, shift)
        scale, shift = rs.gn_affine(y, 32, p[f"conv_layers.{i}.gn.weight"],
                                    p[f"conv_layers.{i}.gn.bias"], 1e-5)
    y_nhwc = y.flatten(2).permute(0, 2, 1)
    f1 = rs.fc_from_conv(y_nhwc, scale, shift, p["fc_layers.0.0.weight"], p["fc_layers.0.0.bias"],
                         True)
    f2 = rs.fc(f1, p["fc_layers.1.0.weight"], p["fc_layers.1.0.bias"], True)
    r, t = rs.heads(f2, p["rotation_pred.weight"], p["rotation_pred.bias"],
                    p["translation_pred.weight"], p["translation_pred.bias"], label, 6)
    assert float((r - r_ref).abs().max()) <= 1e-10
    assert float((t - t_ref).abs().max()) <= 1e-10
    # the channels-last FC1 (permuted weight on the channels-last flatten) is the same layer
    a = torch.relu(y_nhwc * scale[:, None, :] + shift[:, None, :]).reshape(n, -1)
    f1p = rs.fc(a, rs.fc_permute(p["fc_layers.0.0.weight"], 128, 16), p["fc_layers.0.0.bias"], True)
    assert float((f1p - f1).abs().max()) <= 1e-10
    # and the split FC's partial sums recombine to it
    bounds = rs.split_bounds(1024, 4)
    parts = torch.stack([f1[:, lo:hi] @ p["fc_layers.1.0.weight"][:, lo:hi].T for lo, hi in bounds])
    f2s = rs.from_partials(parts, p["fc_layers.1.0.bias"])
    assert float((f2s - f2).abs().max()) <= 1e-10


def test_gn_affine_is_group_norm():
    case = (3, 37, 64, 4)
    parts, gamma, beta = pc.gn_inputs(case)
    y = parts.double().sum(0).permute(0, 2, 1)  # [n, c, hw]
    scale, shift = rs.gn_affine(y, 4, gamma, beta, 1e-5)
    ref = F.group_norm(y, 4, gamma.double(), beta.double(), 1e-5)
    assert float((y * scale[:, :, None] + shift[:, :, None] - ref).abs().max()) <= 1e-12


def test_gn_movement_record():
    """The GroupNorm bound's measured part (posehead_cases' docstring) is what the restatement
    gives on this machine."""
    got = pc.gn_move_bound()
    for g, rec in zip(got, pc.GN_MOVE_RECORDED):
        assert abs(g / rec - 1) < 0.02, (got, pc.GN_MOVE_RECORDED)


NORM_CONVS = [("gather", c, i) for c, i in pc.GATHER_CASES if c[10]] + \
             [("mfma", c, i) for c, i in pc.ENC_CASES if c[8]]


@pytest.mark.parametrize("kind,case", [(k, c) for k, c, _ in NORM_CONVS],
                         ids=[f"{k}-{i}" for k, _, i in NORM_CONVS])
def test_padding_check_has_teeth(kind, case):
    """Norm-on-load next to zero padding, at every normalised conv shape of the GPU tests (gather
    and MFMA form): with shift > 0 on at least half the channels, applying the affine to the
    padded tensor moves the border outputs by more than 100× the GPU conv tolerance and leaves
    every output whose window holds no padding alone — a kernel that normalises its padding
    cannot pass."""
    if kind == "gather":
        n, h, w, c0, c1, cout, k, stride, pad = case[:9]
        d = pc.gather_inputs(case)
    else:
        n, h, w, c0, c1, cout, stride = case[:7]
        k, pad = 3, 1
        d = pc.enc_inputs(case)
    assert float((d["shift"] > 0).float().mean()) >= 0.5
    good = rs.conv(d["x"], d["w"], None, stride, pad, d["scale"], d["shift"])
    bad = affine_on_padding(d["x"], d["w"], stride, pad, d["scale"], d["shift"])
    atol, rtol = pc.conv_tol((c0 + c1) * k * k)
    diff = (good - bad).abs()
    border = border_mask(*good.shape[2:])
    assert float(diff[:, :, border].max()) > 100 * (atol + rtol * float(good.abs().max()))
    assert exceeds(bad, good, atol, rtol)
    is_pad = F.pad(torch.zeros(1, 1, h, w), (pad,) * 4, value=1.0)
    touched = F.max_pool2d(is_pad, k, stride)[0, 0] > 0  # outputs whose window holds padding
    if (~touched).any():
        assert float(diff[:, :, ~touched].max()) == 0


@pytest.mark.parametrize("case", [c for c, _ in pc.ENC_CASES], ids=[i for _, i in pc.ENC_CASES])
def test_conv_slab_partition_sums_to_conv(case):
    """conv_slab over the MFMA conv's stage partition sums to conv (the slab tests' reference is
    consistent with the whole conv's)."""
    n, h, w, cin, cin1, cout, stride, ksplit, norm = case
    d = pc.enc_inputs(case)
    whole = rs.conv(d["x"], d["w"], None, stride, 1, d["scale"], d["shift"])
    total = sum(rs.conv_slab(d["x"], d["w"], stride, 1, d["scale"], d["shift"], 16 * lo, 16 * hi)
                for lo, hi in rs.split_bounds((cin + cin1) // 16, ksplit))
    assert float((total - whole).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", [c for c, _ in pc.GATHER_CASES],
                         ids=[i for _, i in pc.GATHER_CASES])
def test_conv_slab_chunks_partition_sums_to_conv(case):
    """conv_slab_chunks over the gather conv's chunk partition sums to conv — for the cases'
    own splits (72 chunks over 5 cuts inside taps: bounds 14, 28, 43, 57 with 8 chunks per tap)
    and for a split at every single chunk."""
    n, h, w, c0, c1, cout, k, stride, pad, ksplit, norm, bias = case
    d = pc.gather_inputs(case)
    whole = rs.conv(d["x"], d["w"], None, stride, pad, d["scale"], d["shift"])
    nall = rs.chunk_count(c0 + c1, k, k)
    for parts in (ksplit, nall):
        bounds = rs.split_bounds(nall, parts)
        total = sum(rs.conv_slab_chunks(d["x"], d["w"], stride, pad, d["scale"], d["shift"], lo, hi)
                    for lo, hi in bounds)
        assert float((total - whole).abs().max()) <= 1e-12
    if ksplit == 5:
        cch = -(-(c0 + c1) // 16)
        assert any(lo % cch for lo, _ in rs.split_bounds(nall, ksplit))  # cut inside a tap
    # whole-tap slabs are whole-channel convs over a tap subset: tap 0 alone = a 1×1 conv of the
    # padded input's top-left-aligned samples
    cch = nall // (k * k)
    tap0 = rs.conv_slab_chunks(d["x"], d["w"], stride, pad, d["scale"], d["shift"], 0, cch)
    xp = F.pad(rs.norm_on_load(d["x"], d["scale"], d["shift"]), (pad,) * 4)
    oh, ow = whole.shape[2:]
    xs = xp[:, :, 0:(oh - 1) * stride + 1:stride, 0:(ow - 1) * stride + 1:stride]
    ref0 = F.conv2d(xs, d["w"].double()[:, :, :1, :1])
    assert float((tap0 - ref0).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", [c for c, _ in pc.GATHER_CASES if c[9] > 1],
                         ids=[i for c, i in pc.GATHER_CASES if c[9] > 1])
def test_gather_slab_boundary_check_has_teeth(case):
    """A gather-conv slab whose upper bound is off by one chunk fails the slab comparison's
    tolerance at every split GPU case."""
    n, h, w, c0, c1, cout, k, stride, pad, ksplit, norm, bias = case
    d = pc.gather_inputs(case)
    nall = rs.chunk_count(c0 + c1, k, k)
    for lo, hi in rs.split_bounds(nall, ksplit)[:-1]:
        good = rs.conv_slab_chunks(d["x"], d["w"], stride, pad, d["scale"], d["shift"], lo, hi)
        bad = rs.conv_slab_chunks(d["x"], d["w"], stride, pad, d["scale"], d["shift"], lo, hi + 1)
        assert exceeds(bad, good, *pc.conv_tol(rs.chunk_real_k(c0 + c1, k, k, lo, hi)))


@pytest.mark.parametrize("case", [c for c, _ in pc.ENC_CASES if c[7] > 1],
                         ids=[i for c, i in pc.ENC_CASES if c[7] > 1])
def test_enc_slab_boundary_check_has_teeth(case):
    """The same for the MFMA conv's stage slabs (one 16-channel stage)."""
    n, h, w, cin, cin1, cout, stride, ksplit, norm = case
    d = pc.enc_inputs(case)
    for lo, hi in rs.split_bounds((cin + cin1) // 16, ksplit)[:-1]:
        good = rs.conv_slab(d["x"], d["w"], stride, 1, d["scale"], d["shift"], 16 * lo, 16 * hi)
        bad = rs.conv_slab(d["x"], d["w"], stride, 1, d["scale"], d["shift"], 16 * lo, 16 * hi + 16)
        assert exceeds(bad, good, *pc.conv_tol((hi - lo) * 16 * 9))


@pytest.mark.parametrize("m", [3, 33])
@pytest.mark.parametrize("rch", [6, 4])
def test_label0_check_has_teeth(m, rch):
    """Heads that use each row's own label differ from the label[0] heads by more than the heads
    tolerance on every row whose label is not label[0]."""
    x, xb, Wr, br, Wt, bt, label = pc.heads_inputs(40 + m + rch, m, 256, rch)
    r, t = rs.heads(x, Wr, br, Wt, bt, label, rch)
    for i in range(1, m):
        ri, ti = rs.heads(x[i:i + 1], Wr, br, Wt, bt, label[i:i + 1], rch)
        same = int(label[i]) == int(label[0])
        assert exceeds(ri, r[i:i + 1], 1e-6, 1e-5) != same
        assert exceeds(ti, t[i:i + 1], 1e-6, 1e-5) != same
    assert int(label[0]) == 7 and len(set(label.tolist())) > 1
