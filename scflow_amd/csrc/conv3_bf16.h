// Direct 3×3 convolution on bf16 MFMA with fp32 accumulation for the motion encoder's 3×3 convs
// (corr_net.1, flow_net.1, out_net) — the opt-in SCFLOW_CONV_BF16_3X3 format — and, with the fused
// normalisation pieces (NORM, below), for the RAFT encoders' stride-1 3×3 convs — the opt-in
// SCFLOW_CONV_BF16_3X3N format; included by conv.hip (inside its anonymous namespace) after
// conv_bf16_core.h, which holds the halo stager, the packed-weight layout and the rounding.
// Reference: MotionEncoder, models/decoder/raft_decoder.py:75-85 (channel tables), :152-166.
//
// Every buffer stays fp32.  The inputs are rounded to bf16 (round to nearest even) as the halo is
// staged into LDS, the weights when they are packed; a product of two bf16 values is exact in
// fp32 and the accumulators are fp32, so the result is the fp32-accumulated contraction of the
// rounded operands — only the summation order differs from an fp64 evaluation on them.  Bias and
// activation run in fp32 as in the direct fp32 conv.
//
// Implicit GEMM on v_mfma_f32_32x32x16_bf16: M = output pixels, N = output channels, K = 9 taps ×
// (c0 + c1) channels.  Workgroup = 4 rows × 32 columns of one image (128 output pixels; W = 64 has
// two column blocks per row block) × 64 output channels (128 per workgroup measured slower at every
// motion-encoder shape); 4 waves as 2 (M) × 2 (N), each two image rows (two 32-row
// MFMA blocks: a block is one row of 32 pixels) × one 32-channel block.  K is walked in stages of
// 32 channels of one source: the stage's halo (6 rows × 34 columns, pixels outside the image — the
// neighbouring sample's rows included — read as 0) is staged ONCE as bf16 and serves all nine
// taps: tap (ty, tx) reads pixel (y + ty − 1, x + tx − 1) of the same LDS image.  A lane's A
// fragment is 8 consecutive channels of one pixel (one ds_read_b128); pixels are 80 B apart (64 B
// of channels + 16 B pad), so the 16 lanes of every ds_read_b128 lane group — distinct columns mod
// 16 of one row — cover the 16 slots of a bank row (5·l mod 16 is a permutation).  The halo is
// double-buffered: one barrier per stage (36 MFMAs per wave); the next stage's global loads
// (buffer loads) are issued before this stage's MFMAs and rounded into the other buffer after
// them.  Weights are pre-packed bf16 in B-fragment lane order, 1 KiB per (32 output channels,
// 16-channel k-step, tap), streamed from L2 in groups of one tap row (3 taps) of one k-step through
// a ring of three register groups, two groups (12 MFMAs) ahead of their use.  Stores are masked
// per lane to channels < cout (a lane owns one channel of the 32×32 C/D block).  No atomics, a
// fixed summation order: bitwise reproducible.
//
// NORM = true is the RAFT encoder's form (SCFLOW_CONV_BF16_3X3N with a fused pointer set): the
// producer's InstanceNorm + ReLU on load — x' = relu(fmaf(x, in_scale[img][c], in_shift[img][c])),
// one fp32 rounding, applied before the bf16 rounding and only to pixels inside the image, so the
// zero padding (the neighbouring sample's rows included) stays 0 and not relu(in_shift) — and in
// the epilogue the eval-BatchNorm affine and the residual, read with the store's lane map.  A
// thread stages the same 8 channels of every halo pixel, so its scale and shift are 16 registers
// per stage; they are fetched when the stage's halo has been consumed from the staging registers
// (hstore), not with the halo's loads ahead of the MFMAs, where they would be live together with
// the whole weight ring.  NORM = false is the motion encoder's kernel, unchanged.

constexpr int C3OR = 4, C3OC = 32;           // output rows × columns per workgroup
constexpr int C3HR = C3OR + 2, C3HC = C3OC + 2;  // halo
using C3Halo = Bf16Halo<C3HR, C3HC>;  // 816 slots of 8 channels: 4 per thread, the last for 48 threads
constexpr int C3NA = C3Halo::NA;
constexpr int C3BUF = C3Halo::BUF;  // 16-B slots of one LDS halo buffer

struct C3Bf16Params {
  scflow_conv_args a;
  int nst0, nst;  // stages (32 channels) of source 0, of both sources
  int nbt;        // 32-channel blocks of the packed weights (⌈cout / 32⌉)
};

constexpr size_t c3_bf16_lds_bytes() { return C3Halo::LDS_BYTES; }

// (4 waves per SIMD: the grids and times of DESIGN.md §25 rest on four workgroups per CU, so a
// build that needs more than 128 VGPRs must say so instead of halving the occupancy)
template <bool NORM>
__global__ __launch_bounds__(256, 4) void conv3_bf16_kernel(C3Bf16Params P) {
  extern __shared__ floatx4 smem4[];  // 2 × [C3HR·C3HC pixels][SBPITCH] 16-B slots
  const scflow_conv_args& a = P.a;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1, li = lane & 31, hh = lane >> 5;
  const int W = a.w;
  const int XB = W / C3OC;  // column blocks per image row
  const int bx = blockIdx.x, by = blockIdx.y;
  const int blocks_per_img = (a.h / C3OR) * XB;
  const int img = bx / blocks_per_img;
  const int rem = bx - img * blocks_per_img;
  const int oy0 = (rem / XB) * C3OR, ox0 = (rem % XB) * C3OC;
  const int npix = a.n * a.h * W;

  // halo staging (Bf16Halo): the next stage's loads into ra
  int hpix[C3NA];
  C3Halo::pixels(hpix, tid, img, a.h, W, oy0 - 1, ox0 - 1);
  const int hq = tid & 3;
  floatx4 ra[C3NA][2];
  auto hload = [&](int s) { C3Halo::load(ra, hpix, tid, a, P.nst0, npix, s); };
  // stage s's halo from the staging registers into LDS buffer buf
  auto hstore = [&](int buf, int s) {
    if constexpr (NORM) {
      if (a.in_scale) {  // (c1 = 0: every stage is source 0's; workgroup-uniform)
        const size_t c = (size_t)img * a.c0 + s * SBSC + hq * 8;
        const floatx4 sc0 = *(const floatx4*)(a.in_scale + c), sc1 = *(const floatx4*)(a.in_scale + c + 4);
        const floatx4 sh0 = *(const floatx4*)(a.in_shift + c), sh1 = *(const floatx4*)(a.in_shift + c + 4);
#pragma unroll
        for (int j = 0; j < C3NA; ++j) {
          const bool in = hpix[j] >= 0;  // zero padding stays zero (it pads the normalised activation)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            ra[j][0][e] = in ? fmaxf(__builtin_fmaf(ra[j][0][e], sc0[e], sh0[e]), 0.f) : 0.f;
            ra[j][1][e] = in ? fmaxf(__builtin_fmaf(ra[j][1][e], sc1[e], sh1[e]), 0.f) : 0.f;
          }
        }
      }
    }
    C3Halo::store(smem4 + buf * C3BUF, ra, tid);
  };

  // weights [nb32][k-step][tap][lane][8 bf16] (bf16_wblock).  With an odd ⌈cout / 32⌉ the last
  // workgroup's second wave pair has no block of its own: it reads the last packed block again
  // (the block offset is the load's scalar offset, which the buffer's range check does not cover,
  // so it must stay inside the packed weights) and every one of its stores is masked.
  const int nks = P.nst * (SBSC / SBKC);
  const __amdgpu_buffer_rsrc_t wsrc = wino_rsrc(a.weight, (unsigned)((size_t)P.nbt * nks * 9 * 1024));
  const int nb = by * 2 + wn;                     // this wave's 32-channel output block
  const int nbl = nb < P.nbt ? nb : P.nbt - 1;    // the block it loads (wave-uniform)
  const int ngr = nks * 3;                        // weight groups: (k-step, tap row)
  auto uload = [&](floatx4(&u)[3], int g) {
    const int gg = g < ngr ? g : ngr - 1;  // (the last stages re-load the last group)
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) u[tx] = wino_bload(wsrc, lane * 16, bf16_wblock<3>(nbl, ngr, gg, tx));
  };

  // this lane's two A rows (output pixels (2·wm + rb, li) of the block) as halo slot offsets of
  // tap (0, 0), + its channel half
  int abase[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) abase[rb] = ((wm * 2 + rb) * C3HC + li) * SBPITCH + hh;

  floatx16 acc[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[rb][e] = 0.f;

  // the 3 taps of tap row ty of k-step k (0, 1) of the stage in LDS buffer buf
  auto taprow = [&](int buf, int k, int ty, const floatx4(&u)[3]) {
    const floatx4* hb = smem4 + buf * C3BUF + 2 * k + ty * C3HC * SBPITCH;
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
      bf16x8 av[2];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) av[rb] = __builtin_bit_cast(bf16x8, hb[abase[rb] + tx * SBPITCH]);
      const bf16x8 bv = __builtin_bit_cast(bf16x8, u[tx]);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[rb], bv, acc[rb], 0, 0, 0);
    }
  };

  floatx4 u0[3], u1[3], u2[3];  // the ring: group g lives in u(g mod 3)
  uload(u0, 0);
  uload(u1, 1);
  hload(0);
  hstore(0, 0);
  __syncthreads();
  for (int s = 0; s < P.nst; ++s) {
    const int buf = s & 1;
    const int g = 6 * s;
    const bool more = s + 1 < P.nst;  // workgroup-uniform
    if (more) hload(s + 1);
    uload(u2, g + 2);
    taprow(buf, 0, 0, u0);
    uload(u0, g + 3);
    taprow(buf, 0, 1, u1);
    uload(u1, g + 4);
    taprow(buf, 0, 2, u2);
    uload(u2, g + 5);
    taprow(buf, 1, 0, u0);
    uload(u0, g + 6);
    taprow(buf, 1, 1, u1);
    uload(u1, g + 7);
    taprow(buf, 1, 2, u2);
    if (more) hstore(buf ^ 1, s + 1);  // its readers finished with buf ^ 1 before the last barrier
    __syncthreads();
  }

  // epilogue; C/D layout: col = lane&31, row = mfma32_row — the direct conv's (conv_mfma_kernel),
  // with its arithmetic.  A lane writes its own channel only: nothing at or
  // past cout of the destination's pixel stride is touched.
  const int col = nb * 32 + li;
  if (col >= a.cout) return;
  const float bias = a.bias ? a.bias[col] : 0.f;
  if constexpr (NORM) {
    // v = conv + bias; the eval-BatchNorm affine; the residual (this lane's channel of the pixels
    // it stores, read before any of them is written: res may be the output); the activation
    const bool aff = a.out_scale != nullptr;
    const float osc = aff ? a.out_scale[col] : 1.f;
    const float osh = aff ? a.out_shift[col] : 0.f;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const size_t row0 = (size_t)(img * a.h + oy0 + wm * 2 + rb) * W + ox0;
      float rv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int x = mfma32_row(r, hh);
        rv[r] = a.res ? a.res[(row0 + x) * a.sres + col] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int x = mfma32_row(r, hh);
        float v = acc[rb][r] + bias;
        if (aff) v = v * osc + osh;
        if (a.res) v += rv[r];
        a.out[(row0 + x) * a.so + col] = act_apply(v, a.act);
      }
    }
    return;
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const size_t row0 = (size_t)(img * a.h + oy0 + wm * 2 + rb) * W + ox0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int x = mfma32_row(r, hh);
      a.out[(row0 + x) * a.so + col] = act_apply(acc[rb][r] + bias, a.act);
    }
  }
}
