// Direct 1×5 / 5×1 convolution on bf16 MFMA with fp32 accumulation for the SeqConv GRU — the
// opt-in SCFLOW_CONV_BF16 format; included by conv.hip (inside its anonymous namespace) after
// conv_bf16_core.h, which holds the halo stager, the packed-weight layout and the rounding.
// Reference: ConvGRU SeqConv, models/decoder/raft_decoder.py:180-181 (kernel table), :235-253.
//
// Every buffer stays fp32.  The inputs are rounded to bf16 (round to nearest even) as the halo is
// staged into LDS, the weights when they are packed; a product of two bf16 values is exact in
// fp32 and the accumulators are fp32, so the result is the fp32-accumulated contraction of the
// rounded operands — only the summation order differs from an fp64 evaluation on them.  Bias,
// bias map, activation and the GRU epilogues run in fp32 as in the direct fp32 conv.
//
// Implicit GEMM on v_mfma_f32_32x32x16_bf16: M = output pixels, N = output channels, K = 5 taps ×
// (c0 + c1) channels.  Workgroup = Wino5Geom's block (128 output pixels: 128/W whole rows for 1×5,
// 4 rows × 32 columns for 5×1) × 64·NBW output channels; 4 waves as 2 (M) × 2 (N), each 64 pixels
// (two 32-row blocks) × NBW 32-channel blocks.  K is walked in stages of 32 channels of one source:
// the stage's halo (rows + 4 or columns + 4) is staged ONCE as bf16 and serves all five taps — tap
// t reads pixel x + t − 2 (row y + t − 2) of the same LDS image.  A lane's A fragment is 8
// consecutive channels of one pixel (one ds_read_b128); pixels are 80 B apart (64 B of channels +
// 16 B pad), so the 16 lanes of every ds_read_b128 lane group — consecutive pixels of one row —
// cover the 16 slots of a bank row (5·l mod 16 is a permutation).  The halo is double-buffered:
// one barrier per stage (40·NBW MFMAs per wave); the next stage's global loads (buffer loads,
// out-of-image pixels read as 0) are issued before this stage's MFMAs and rounded into the other
// buffer after them.  Weights are pre-packed bf16 in B-fragment lane order, 1 KiB per (32 output
// channels, 16-channel k-step, tap), streamed from L2 one k-step (5 taps) ahead of their MFMAs.
// No atomics, a fixed summation order: bitwise reproducible.

struct SepBf16Params {
  scflow_conv_args a;
  int nst0, nst;               // stages (32 channels) of source 0, of both sources
  unsigned long long* stamps;  // profiling (scflow_debug_conv_stamps), or NULL
};

template <int DIR, int W>
using SepBf16Halo = Bf16Halo<Wino5Geom<DIR, W>::HR, Wino5Geom<DIR, W>::HC>;
template <int DIR, int W>
constexpr size_t sep_bf16_lds_bytes() {
  return SepBf16Halo<DIR, W>::LDS_BYTES;
}

template <int DIR, int W, int NBW, int EPI>  // DIR 0: 1×5 (along x), 1: 5×1 (along y)
__global__ __launch_bounds__(256, 2) void conv_sep_bf16_kernel(SepBf16Params P) {
  using G = Wino5Geom<DIR, W>;
  using H = SepBf16Halo<DIR, W>;
  extern __shared__ floatx4 smem4[];  // 2 × [HR·HC pixels][SBPITCH] 16-B slots
  const scflow_conv_args& a = P.a;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1, li = lane & 31, hh = lane >> 5;
  constexpr int XB = W / G::OCOLS;  // column blocks per image (1, or 2 for 5×1 at W = 64)
  const int bx = blockIdx.x, by = blockIdx.y;
  wino_stamp(P.stamps, 0);
  const int blocks_per_img = (a.h / G::OROWS) * XB;
  const int img = bx / blocks_per_img;
  const int rem = bx % blocks_per_img;
  const int oy0 = (rem / XB) * G::OROWS, ox0 = (rem % XB) * G::OCOLS;
  const int npix = a.n * a.h * W;
  const int hy0 = DIR == 0 ? oy0 : oy0 - 2, hx0 = DIR == 0 ? -2 : ox0;  // halo origin

  // halo staging (Bf16Halo): the next stage's loads into ra, ra rounded into LDS buffer buf
  int hpix[H::NA];
  H::pixels(hpix, tid, img, a.h, W, hy0, hx0);
  floatx4 ra[H::NA][2];
  auto hload = [&](int s) { H::load(ra, hpix, tid, a, P.nst0, npix, s); };
  auto hstore = [&](int buf) { H::store(smem4 + buf * H::BUF, ra, tid); };

  // weights [nb32][k-step][tap][lane][8 bf16] (bf16_wblock)
  const int nks = P.nst * (SBSC / SBKC);
  const int nbt = (int)gridDim.y * 2 * NBW;  // 32-channel blocks packed
  const __amdgpu_buffer_rsrc_t wsrc = wino_rsrc(a.weight, (unsigned)((size_t)nbt * nks * 5 * 1024));
  const int nb0 = (by * 2 + wn) * NBW;
  auto uload = [&](floatx4(&u)[5][NBW], int ks) {
    const int kk = ks < nks ? ks : nks - 1;
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
      for (int nb = 0; nb < NBW; ++nb)
        u[t][nb] = wino_bload(wsrc, lane * 16, bf16_wblock<5>(nb0 + nb, nks, kk, t));
  };

  // this lane's two A rows (output pixels) as halo slot offsets (tap 0), + its channel half
  int abase[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int m = wm * 64 + rb * 32 + li;
    abase[rb] = ((m / G::OCOLS) * G::HC + m % G::OCOLS) * SBPITCH + hh;
  }
  constexpr int TAPP = (DIR == 0 ? 1 : G::HC) * SBPITCH;  // slots between taps

  floatx16 acc[2][NBW];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[rb][nb][e] = 0.f;

  // the 5 taps of k-step k (0, 1) of the stage in LDS buffer buf
  auto kstep = [&](int buf, int k, const floatx4(&u)[5][NBW]) {
    const floatx4* hb = smem4 + buf * H::BUF + 2 * k;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      bf16x8 av[2];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) av[rb] = __builtin_bit_cast(bf16x8, hb[abase[rb] + t * TAPP]);
#pragma unroll
      for (int nb = 0; nb < NBW; ++nb) {
        const bf16x8 bv = __builtin_bit_cast(bf16x8, u[t][nb]);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
          acc[rb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[rb], bv, acc[rb][nb], 0, 0, 0);
      }
    }
  };

  floatx4 uA[5][NBW], uB[5][NBW];
  uload(uA, 0);
  hload(0);
  hstore(0);
  __syncthreads();
  wino_stamp(P.stamps, 1);
  for (int s = 0; s < P.nst; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < P.nst;  // workgroup-uniform
    if (more) hload(s + 1);
    uload(uB, 2 * s + 1);
    kstep(buf, 0, uA);
    uload(uA, 2 * s + 2);
    kstep(buf, 1, uB);
    if (more) hstore(buf ^ 1);  // its readers finished with buf ^ 1 before the last barrier
    __syncthreads();
  }
  wino_stamp(P.stamps, 2);

  // epilogue; C/D layout: col = lane&31, row = mfma32_row — the direct conv's (conv_mfma_kernel),
  // with its arithmetic.  Per 32×32 block, all global reads (bias map, h, z)
  // before any store.
#pragma unroll
  for (int nb = 0; nb < NBW; ++nb) {
    const int col = (nb0 + nb) * 32 + li;
    if (col >= a.cout) continue;
    const float bias = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      size_t pixv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = wm * 64 + rb * 32 + mfma32_row(r, hh);
        pixv[r] = (size_t)((img * a.h + oy0 + m / G::OCOLS) * W + ox0 + m % G::OCOLS);
      }
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = acc[rb][nb][r];
      if (a.bias_map) {
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] += a.bias_map[pixv[r] * a.sbm + col];
      }
      if constexpr (EPI == SCFLOW_EPI_PLAIN) {
#pragma unroll
        for (int r = 0; r < 16; ++r) a.out[pixv[r] * a.so + col] = act_apply(v[r] + bias, a.act);
      } else if constexpr (EPI == SCFLOW_EPI_GRU_ZR) {
        const int hcn = a.cout >> 1;
        if (col < hcn) {
#pragma unroll
          for (int r = 0; r < 16; ++r) a.gate[pixv[r] * a.sg + col] = sigmoidf_(v[r] + bias);
        } else {
          const int c = col - hcn;
          float hv[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) hv[r] = a.hid[pixv[r] * a.sh + c];
#pragma unroll
          for (int r = 0; r < 16; ++r) a.rh[pixv[r] * a.srh + c] = sigmoidf_(v[r] + bias) * hv[r];
        }
      } else {  // GRU_Q
        float zv[16], hv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          zv[r] = a.gate[pixv[r] * a.sg + col];
          hv[r] = a.hid[pixv[r] * a.sh + col];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float q = tanhf_(v[r] + bias);
          a.hid[pixv[r] * a.sh + col] = (1.f - zv[r]) * hv[r] + zv[r] * q;
        }
      }
    }
  }
  if (P.stamps) {
    __builtin_amdgcn_s_waitcnt(0);
    wino_stamp(P.stamps, 3);
  }
}
