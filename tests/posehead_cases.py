"""Test-side helper (not a test): the shapes, seeded inputs and tolerances that the pose head's
CPU and GPU tests share (``tests/test_posehead_host.py``, ``tests/test_gpu_posehead_ops.py``).
Plain torch on the CPU; the reference arithmetic is ``tests/posehead_restatement.py``.

Tolerances
* convs and FCs: the project's fp32 bound (``test_conv2d_variants``), atol = 2e-6·√K·4 with
  rtol = 1e-5, K the length of the sum the compared element covers (a slab: the slab's own K);
* ``scflow_ph_gn_reduce``'s slab sum y: (nsplit−1)·2⁻²⁴·Σ_z|part_z| per element (a chain of
  nsplit−1 fp32 additions);
* its scale / shift: the statistics accumulate in fp64, so what is left is the fp32 rounding of
  y, the casts of mean and rstd and two fp32 operations.  ``gn_movement`` measures, from the
  restatement alone, how far ``gn_affine`` moves when the exact fp64 slab sum is replaced by the
  sum accumulated in fp32 (forward and reverse slab order); the bound is 4× the largest movement
  over ``GN_CASES`` plus 4 fp32 ulps of the larger of the result and, for shift, |β| and
  |mean·scale|.  Measured over ``GN_CASES`` with these seeds: scale moves by at most 2.03e-08,
  shift by at most 6.54e-08 (``GN_MOVE_RECORDED``; ``test_posehead_host.py`` re-measures and
  checks the record), so the constant part of the bound is 8.1e-08 for scale and 2.6e-07 for
  shift;
* heads: ``test_pose_step_heads_fused``'s rtol 1e-5, atol 1e-6.
"""
from functools import lru_cache

import numpy as np
import torch

from tests import posehead_restatement as rs

SENTINEL = 777.0

# ---------------------------------------------------------------------------------- convs
# (n, h, w, c0, c1, cout, k, stride, pad, ksplit, norm, bias)
GATHER_CASES = [
    ((1, 8, 8, 128, 0, 128, 3, 2, 1, 4, True, False), "b1-conv3-M16-under-one-tile"),
    ((3, 8, 8, 128, 0, 128, 3, 2, 1, 5, True, False), "M48-ragged-tile-72chunks-over-5"),
    ((5, 8, 8, 128, 0, 128, 3, 2, 1, 1, False, True), "M80-unsplit-bias"),
    ((2, 9, 7, 20, 8, 40, 3, 2, 1, 2, True, False), "odd-two-sources-cin28-cout40"),
    ((2, 6, 10, 16, 0, 33, 1, 1, 0, 1, False, True), "1x1-stride1-cout33"),
    ((1, 5, 5, 16, 0, 8, 3, 1, 1, 9, False, False), "one-chunk-per-slice"),
]

# (n, h, w, cin, cin1, cout, stride, ksplit, norm); 3×3, pad 1; ksplit = 1 runs with bias + ReLU
ENC_CASES = [
    ((1, 32, 32, 128, 96, 128, 2, 14, False), "b1-conv1-one-stage-per-slice"),
    ((3, 32, 32, 128, 96, 128, 2, 5, False), "14-stages-over-5-uneven"),
    ((2, 16, 16, 128, 0, 128, 2, 8, True), "conv2-norm"),
    ((2, 16, 16, 32, 16, 80, 2, 3, True), "last-slab-all-src1-scale-table-across-sources-cout80"),
    ((1, 8, 16, 16, 16, 64, 1, 2, True), "stride1-tile"),
    ((2, 16, 16, 32, 16, 64, 2, 1, True), "unsplit-bias-relu"),
]


def conv_tol(K):
    """(atol, rtol) of a conv / FC output that sums K products."""
    return 2e-6 * float(np.sqrt(K)) * 4, 1e-5


def conv_inputs(seed, n, h, w, cin, cout, k, norm=True, bias=True):
    """x [n, cin, h, w], w [cout, cin, k, k] scaled by 1/√fan-in, bias, and the input GroupNorm's
    per-(sample, channel) scale / shift: shift has mixed signs and is positive on every even
    channel (so at least half of them turn zero padding into relu(shift) > 0 if the affine is
    wrongly applied to it)."""
    g = torch.Generator().manual_seed(seed)
    d = dict(x=torch.randn(n, cin, h, w, generator=g),
             w=torch.randn(cout, cin, k, k, generator=g) / float(np.sqrt(cin * k * k)),
             bias=0.1 * torch.randn(cout, generator=g) if bias else None, scale=None, shift=None)
    if norm:
        d["scale"] = 0.5 * torch.randn(n, cin, generator=g) + 1.0
        sh = 0.5 * torch.randn(n, cin, generator=g)
        sh[:, ::2] = sh[:, ::2].abs() + 0.1
        d["shift"] = sh
    return d


def gather_inputs(case):
    n, h, w, c0, c1, cout, k, stride, pad, ksplit, norm, bias = case
    return conv_inputs(1000 + 7 * n + h + c0, n, h, w, c0 + c1, cout, k, norm, bias)


def enc_inputs(case):
    n, h, w, cin, cin1, cout, stride, ksplit, norm = case
    return conv_inputs(2000 + 7 * n + h + cin + ksplit, n, h, w, cin + cin1, cout, 3, norm,
                       ksplit == 1)


# ---------------------------------------------------------------------------------- GroupNorm
GN_N, GN_EPS = 3, 1e-5
# (nsplit, hw, c, groups).  nsplit 1, 2, 3, 4, 8: compile-time slab counts; 5, 14: the generic
# loop.  hw 16: tail loop only, most pixel slots idle; 256: exactly one unrolled round; 300:
# unrolled round + ragged tail; 37: ragged tail only.  groups 2 of 64 channels: 32-channel blocks.
GN_CASES = [(ns, hw, 128, 32) for ns in (1, 2, 3, 4, 8, 5, 14) for hw in (16, 300)] + [
    (4, 256, 128, 32), (3, 256, 128, 32), (8, 256, 128, 32), (14, 256, 128, 32),
    (2, 37, 128, 32), (5, 37, 128, 32),
    (3, 300, 64, 4), (14, 16, 64, 4),
    (1, 300, 64, 2), (4, 300, 64, 2), (5, 37, 64, 2), (8, 16, 64, 2),
    (2, 256, 32, 32), (3, 37, 32, 32),
]
GN_CB32_CASES = [(4, 300, 128, 32), (5, 16, 128, 32)]  # repeated with SCFLOW_GNR_CB=32
GN_MOVE_RECORDED = (2.03e-08, 6.54e-08)  # measured max movement of (scale, shift) over GN_CASES


def gn_inputs(case):
    """parts [nsplit, n, hw, c] (nonzero mean), γ, β."""
    ns, hw, c, groups = case
    g = torch.Generator().manual_seed(3000 + 131 * ns + 7 * hw + c + groups)
    parts = torch.randn(ns, GN_N, hw, c, generator=g) * 2 + 0.5
    return parts, torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)


def _nchw(y_nhwc):  # [n, hw, c] → [n, c, hw]
    return y_nhwc.permute(0, 2, 1)


def gn_reference(case):
    """fp64: the slab sum [n, hw, c], its elementwise fp32-summation bound, (scale, shift)."""
    parts, gamma, beta = gn_inputs(case)
    y = parts.double().sum(0)
    ybound = (parts.shape[0] - 1) * 2.0 ** -24 * parts.double().abs().sum(0)
    return y, ybound, rs.gn_affine(_nchw(y), case[3], gamma, beta, GN_EPS)


def gn_movement(case):
    """How far gn_affine's (scale, shift) move between the exact fp64 slab sum and the slab sum
    accumulated in fp32, in forward and in reverse slab order: (max |Δscale|, max |Δshift|)."""
    parts, gamma, beta = gn_inputs(case)
    exact = rs.gn_affine(_nchw(parts.double().sum(0)), case[3], gamma, beta, GN_EPS)
    ms = mh = 0.0
    for order in (range(parts.shape[0]), reversed(range(parts.shape[0]))):
        acc = None
        for z in order:
            acc = parts[z].clone() if acc is None else acc + parts[z]  # fp32 additions
        sc, sh = rs.gn_affine(_nchw(acc), case[3], gamma, beta, GN_EPS)
        ms = max(ms, float((sc - exact[0]).abs().max()))
        mh = max(mh, float((sh - exact[1]).abs().max()))
    return ms, mh


@lru_cache(maxsize=None)
def gn_move_bound():
    """The largest movement over GN_CASES: (scale, shift)."""
    mv = [gn_movement(c) for c in GN_CASES]
    return max(m[0] for m in mv), max(m[1] for m in mv)


def ulp32(v):
    """One fp32 unit in the last place at |v| (fp64 tensor)."""
    a = v.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def gn_tolerances(case):
    """Elementwise bounds (scale, shift) [n, c] for the case (module docstring)."""
    _, gamma, beta = gn_inputs(case)
    _, _, (scale, shift) = gn_reference(case)
    ms, mh = gn_move_bound()
    mean_scale = beta.double()[None, :] - shift
    big = torch.maximum(shift.abs(), torch.maximum(beta.double().abs()[None, :].expand_as(shift),
                                                   mean_scale.abs()))
    return 4 * ms + 4 * ulp32(scale), 4 * mh + 4 * ulp32(big)


# ---------------------------------------------------------------------------------- FCs, heads
def fc_inputs(seed, m, k, n):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / float(np.sqrt(k)),
            0.1 * torch.randn(n, generator=g))


HEAD_LABELS = [7, 3, 12, 0, 20, 5, 9]  # label[0] = 7 for every sample; all < 21


def heads_inputs(seed, m, k, rch, ncls=21, xsplit=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((xsplit, m, k) if xsplit else (m, k), generator=g)
    xb = 0.1 * torch.randn(k, generator=g)
    Wr = torch.randn(rch * ncls, k, generator=g) / float(np.sqrt(k))
    br = 0.1 * torch.randn(rch * ncls, generator=g)
    Wt = torch.randn(3 * ncls, k, generator=g) / float(np.sqrt(k))
    bt = 0.1 * torch.randn(3 * ncls, generator=g)
    label = torch.tensor([HEAD_LABELS[i % len(HEAD_LABELS)] for i in range(m)], dtype=torch.int64)
    return x, xb, Wr, br, Wt, bt, label
