// Grouped launches of two independent convolutions (round 6) — included by conv.hip (in an
// anonymous namespace).  The decoder's iteration tail runs two short branches side by side — the
// flow predictor → Δflow encoder (3×3 256→2, 7×7 2→128, 3×3 128→64) and the mask predictor → mask
// encoder (1×1 256→1, 3×3 1→64, 3×3 64→32) (scflow_decoder.py:211-218).  Each of those launches
// is a one-round grid of at most one workgroup per CU, and the branches ran on two HIP streams
// joined by events whose fork and join cost 5–10 µs of queue time each.  Pairing the branches'
// k-th launches into ONE grid — workgroups [0, n_a) run conv a's body, the rest conv b's — keeps
// both on one stream with no events and gives each CU a second workgroup.  A pair is chosen from
// the two convs' launch plans (plan_conv, conv.hip) — the kernel family, instantiation, grid and LDS
// that scflow_conv2d itself launches from — and each half runs that instantiation's body on that
// grid, so there is no second copy of the eligibility rules to drift and the results are
// bit-identical to two separate launches.

// thin: the flow predictor's 3×3 contraction (conv_thinz.h) beside the mask predictor's 1×1
// chunked kernel
template <int W, int R>
__global__ __launch_bounds__(256, 2) void thin_pair_kernel(scflow_conv_args f, scflow_conv_args m,
                                                           int oh, int ow, int nf) {
  if ((int)blockIdx.x < nf)
    conv_thinz_body<2, 3, 3, W, R>(f, blockIdx.x, nf);
  else
    conv_thin_body<1, 1, 1>(m, oh, ow, (int)blockIdx.x - nf, (int)gridDim.x - nf);
}

// small-cin: the Δflow encoder's 7×7 2→128 beside the mask encoder's 3×3 1→64
__global__ __launch_bounds__(256, 2) void smallcin_pair_kernel(scflow_conv_args a, scflow_conv_args b,
                                                               int oh, int ow, int na, int nta,
                                                               int ntb, unsigned long long* stamps) {
  if ((int)blockIdx.x < na)
    conv_smallcin_mfma_body<2, 7, 7, 2>(a, oh, ow, 128, nta, blockIdx.x, na, 0, stamps, blockIdx.x);
  else
    conv_smallcin_mfma_body<1, 3, 3, 1>(b, oh, ow, 64, ntb, (int)blockIdx.x - na,
                                        (int)gridDim.x - na, 0, stamps, blockIdx.x);
}

// F(2×2,3×3): two Winograd convs of one width (the encoders' second layers), logical grids
// gxa × gya and gxb × gyb flattened
template <int W, int NA, int NB>
__global__ __launch_bounds__(256, 2) void wino_pair_kernel(WinoParams pa, WinoParams pb, int gxa,
                                                           int gya, int gxb, int gyb) {
  const int L = blockIdx.x, na = gxa * gya;
  if (L < na)
    conv_wino_body<W, NA, false>(pa, L % gxa, L / gxa, gxa, gya, L);
  else
    conv_wino_body<W, NB, false>(pb, (L - na) % gxb, (L - na) / gxb, gxb, gyb, L);
}

// The grouped kernel that covers (a, b) in this order, or SCFLOW_PAIR_NONE: decided on the two
// launch plans alone (plus the shapes the two halves must share).
int pair_kind(const scflow_conv_args& a, const ConvPlan& pa, const scflow_conv_args& b,
              const ConvPlan& pb) {
  if (!pair_enabled()) return SCFLOW_PAIR_NONE;
  // thin: a = 3×3 → 2 contraction, b = 1×1 → 1 chunked
  if (pa.kind == SCFLOW_PLAN_THINZ && a.cout == 2 && pb.kind == SCFLOW_PLAN_THIN_CHUNKED &&
      b.cout == 1 && b.kh == 1 && b.kw == 1 && b.c1 == 0 && a.n == b.n && a.h == b.h && a.w == b.w)
    return SCFLOW_PAIR_THIN;
  // small-cin: a = 7×7 2 → 128 (one workgroup per tile), b = 3×3 1 → 64
  if (pa.kind == SCFLOW_PLAN_SMALLCIN_MFMA && pb.kind == SCFLOW_PLAN_SMALLCIN_MFMA && a.c0 == 2 &&
      a.kh == 7 && pa.nbw == 2 && b.c0 == 1 && pb.npad == 64 && a.h == b.h && a.w == b.w)
    return SCFLOW_PAIR_SMALLCIN;
  // F(2×2,3×3) of one width, 32 or 64 output channels per workgroup, neither with the input
  // affine (the pair runs the bodies without it; the encoders' convs go out one by one)
  if (pa.kind == SCFLOW_PLAN_WINO && pb.kind == SCFLOW_PLAN_WINO && a.w == b.w && a.w != 128 &&
      pa.nbw <= 2 && pb.nbw <= 2 && !a.in_scale && !b.in_scale)
    return SCFLOW_PAIR_WINO;
  return SCFLOW_PAIR_NONE;
}

template <int W, int NA, int NB>
int launch_wino_pair(const WinoParams& wa, const WinoParams& wb, const ConvPlan& pa,
                     const ConvPlan& pb, hipStream_t st) {
  const size_t la = wino_lds_bytes<W, NA>(), lb = wino_lds_bytes<W, NB>();
  const size_t lds = la > lb ? la : lb;
  allow_big_lds<wino_pair_kernel<W, NA, NB>>(lds);
  wino_pair_kernel<W, NA, NB><<<pa.gx * pa.gy + pb.gx * pb.gy, 256, lds, st>>>(
      wa, wb, (int)pa.gx, (int)pa.gy, (int)pb.gx, (int)pb.gy);
  return scflow_launch_status();
}
template <int W>
int launch_wino_pair_w(const WinoParams& wa, const WinoParams& wb, const ConvPlan& pa,
                       const ConvPlan& pb, hipStream_t st) {
  if (pa.nbw == 1)
    return pb.nbw == 1 ? launch_wino_pair<W, 1, 1>(wa, wb, pa, pb, st)
                       : launch_wino_pair<W, 1, 2>(wa, wb, pa, pb, st);
  return pb.nbw == 1 ? launch_wino_pair<W, 2, 1>(wa, wb, pa, pb, st)
                     : launch_wino_pair<W, 2, 2>(wa, wb, pa, pb, st);
}

// the grouped launch pair_kind chose for (a, b): workgroups, tiles and LDS are the two plans'
int launch_pair(int kind, const scflow_conv_args& a, const ConvPlan& pa, const scflow_conv_args& b,
                const ConvPlan& pb, hipStream_t st) {
  const unsigned blocks = pa.gx + pb.gx;
  if (kind == SCFLOW_PAIR_THIN) {  // the 1×1 half's LDS (the contraction uses none)
    if (pa.ow == 64)
      thin_pair_kernel<64, 4><<<blocks, 256, pb.lds, st>>>(a, b, pb.oh, pb.ow, (int)pa.gx);
    else
      thin_pair_kernel<32, 2><<<blocks, 256, pb.lds, st>>>(a, b, pb.oh, pb.ow, (int)pa.gx);
    return scflow_launch_status();
  }
  if (kind == SCFLOW_PAIR_SMALLCIN) {
    smallcin_pair_kernel<<<blocks, 256, pa.lds > pb.lds ? pa.lds : pb.lds, st>>>(
        a, b, pa.oh, pa.ow, (int)pa.gx, pa.ntiles, pb.ntiles, g_wino_stamps);
    return scflow_launch_status();
  }
  // swz_c = 0: the logical grid is not dealt to XCDs in linear order here (block order only)
  const WinoParams wa{a, pa.cp0, pa.nst, 0, g_wino_stamps}, wb{b, pb.cp0, pb.nst, 0, g_wino_stamps};
  return a.w == 32 ? launch_wino_pair_w<32>(wa, wb, pa, pb, st)
                   : launch_wino_pair_w<64>(wa, wb, pa, pb, st);
}
