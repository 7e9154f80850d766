// 1-D Winograd F(4, 5) convolution on fp32 MFMA for the SeqConv GRU's 1×5 and 5×1 convs —
// included by conv.hip (inside its anonymous namespace).  Reference: ConvGRU SeqConv,
// models/decoder/raft_decoder.py:180-181 (kernel table), :235-253 (z, r, q gates).
//
// A tile is 4 consecutive output pixels along the conv axis; its 8 input pixels d give
//   y = Aᵀ[(G g) ⊙ (Bᵀ d)],   transform points {0, ±1, ±2, ±½, ∞},
// i.e. 8 multiplies per tile instead of 20 (2.5× less matrix work).  The coefficients are the
// exact rationals of the Toom-Cook construction; the fp32 error of the whole conv measured in a
// numpy restatement (384 channels) is 2.0× that of the direct fp32 conv — the same order, far
// inside the decoder's tolerances.  The weight transform is done in fp64 once per packing.
//
// Per transform point ξ the channel contraction is a GEMM M_ξ[tile][co] = Σ_ci V_ξ·U_ξ on
// v_mfma_f32_32x32x2_f32.  Workgroup = 32 tiles (128 output pixels: 128/W whole rows for 1×5,
// a 4-row × 32-column block for 5×1) × 32·NBW output channels, 4 waves.  The points are paired
// by the symmetry of Bᵀ: waves 0-2 own (1,2), (3,4), (5,6), whose rows are b ± a with a the odd
// and b the even taps (7 packed float4 ops per 8 channels for both points), wave 3 owns (0,7).
// Each wave forms its two rows of Bᵀd straight into registers from the input halo in LDS and
// streams its points' pre-transformed weights from L2 (lane-ordered, one 1 KiB buffer load per
// point, 8 channels and 32 output channels, reloaded as soon as its MFMAs are issued).  The halo
// ((rows + 4 or + 0) × (columns + 4 or + 0) pixels × 32 channels per stage) is double-buffered
// in LDS: one barrier per stage (64 MFMAs per wave), the next stage's halo loaded and stored in
// halves between this stage's two 16-channel sub-steps, the next sub-step's input transform
// computed between this sub-step's MFMAs, every global load a buffer load (see conv_wino.h on
// why VALU work in the loop matters).  The epilogue gathers the 8 points of every (tile,
// channel) in LDS, applies Aᵀ and runs the same fused epilogues as the direct conv (bias map,
// bias + activation, GRU z | r·h, GRU h ← (1−z)h + z·tanh(q)).

constexpr int W5KC = 16;  // input channels per sub-step
constexpr int W5SC = 32;  // input channels per stage (one LDS halo buffer)
constexpr int W5NSUB = W5SC / W5KC;
constexpr int W5TM = 32;  // tiles per workgroup

constexpr float kW5AT[4][8] = {{1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 0.0f},
                               {0.0f, 1.0f, -1.0f, 2.0f, -2.0f, 0.5f, -0.5f, 0.0f},
                               {0.0f, 1.0f, 1.0f, 4.0f, 4.0f, 0.25f, 0.25f, 0.0f},
                               {0.0f, 1.0f, -1.0f, 8.0f, -8.0f, 0.125f, -0.125f, 1.0f}};
// the transform point held in slot x (0, 1) of wave w
__host__ __device__ constexpr int w5_point(int w, int x) {
  return w == 3 ? (x == 0 ? 0 : 7) : 2 * w + 1 + x;
}

struct Wino5Params {
  scflow_conv_args a;
  int cp0, nst;  // source 0's channels padded to W5SC, stages (W5SC channels each) over both
  int swz_c;     // XCD-aware block order (wino_block, conv_wino.h), 0 = off
  unsigned long long* stamps;  // profiling (scflow_debug_conv_stamps, conv_wino.h), or NULL
};

template <int DIR, int W>  // DIR 0: 1×5 (along x), 1: 5×1 (along y)
struct Wino5Geom {
  static constexpr int TPR = DIR == 0 ? W / 4 : 32;     // tiles per row of the block
  static constexpr int OROWS = DIR == 0 ? 128 / W : 4;  // output rows per workgroup
  static constexpr int OCOLS = DIR == 0 ? W : 32;       // output columns per workgroup
  static constexpr int HR = DIR == 0 ? OROWS : OROWS + 4;
  static constexpr int HC = DIR == 0 ? W + 4 : 32;
  static constexpr int NH4 = HR * HC * (W5SC / 4);  // float4 of one stage's halo
  static constexpr int NA = (NH4 + 511) / 512;      // float4 per thread per half stage
  // LDS halo layout (float4 units): 8 per pixel, one more every SK pixels and a row pad, chosen
  // (exhaustive bank model, tools/dbg/lds_banks.py) so that each of ds_read_b128's four 16-lane
  // groups — lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same +32 (MI355X_MICROARCH.md
  // §LDS), not 16 consecutive lanes — reads 16 distinct 16-B slots of the 256-B bank row.  1×5:
  // a lane group spans 2-4 tile rows, so the row pitch matters (≡ 8 mod 16 float4 after the skew);
  // 5×1: one tile row, the per-pixel skew alone separates the columns.
  static constexpr int SK = DIR == 0 ? 4 : 2;
  static constexpr int ROWP = HC * 8 + HC / SK + (DIR == 0 ? 15 : 0);
  static constexpr int BUF4 = HR * ROWP;
  __device__ static constexpr int addr(int r, int c) { return r * ROWP + c * 8 + c / SK; }
};

template <int DIR, int W, int NBW>
constexpr size_t wino5_lds_bytes() {
  const size_t halo = (size_t)2 * Wino5Geom<DIR, W>::BUF4 * 4;  // double-buffered
  const size_t epi = (size_t)8 * (W5TM + 4) * 32 * NBW;
  return sizeof(float) * (halo > epi ? halo : epi);
}

// (A K split for the GRU q conv's one-workgroup-per-CU grid — two wave sets over the two 8-channel
// halves of every sub-step — was built in round 4 and measured in round 5: 32.7 → 32.5 µs alone,
// the decoder 2 % slower; removed.)
// (Paired workgroups — two tile blocks per 512-thread workgroup meeting at every barrier, so the
// SQ's oldest-first issue cannot let the first-dispatched workgroup of a CU run ahead of the
// second — were measured in round 5: both main loops then take what the second one took alone,
// 42 µs for z|r, and the decoder ran 1 % slower; removed.)
template <int DIR, int W, int NBW, int EPI>
__global__ __launch_bounds__(256, 2) void conv_wino5_kernel(Wino5Params P) {
  using G = Wino5Geom<DIR, W>;
  constexpr int NTH = 256;                                   // threads
  constexpr int NA = (G::NH4 + 2 * NTH - 1) / (2 * NTH);    // float4 per thread per half stage
  constexpr int BNW = 32 * NBW;
  extern __shared__ floatx4 smem4[];
  float* smem = (float*)smem4;
  const scflow_conv_args& a = P.a;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar operands
  const int wave = wv & 3;              // point pair
  const int li = lane & 31, hh = lane >> 5;
  constexpr int XB = W / G::OCOLS;  // column blocks per image (1, or 2 for 5×1 at W = 64)
  int bx, by;
  wino_block(P.swz_c, bx, by);
  wino_stamp(P.stamps, 0);
  const int blocks_per_img = (a.h / G::OROWS) * XB;
  const int img = bx / blocks_per_img;
  const int rem = bx % blocks_per_img;
  const int oy0 = (rem / XB) * G::OROWS, ox0 = (rem % XB) * G::OCOLS;
  const int nst0 = P.cp0 / W5SC;
  const int nst = P.nst;
  const int npix = a.n * a.h * W;
  // halo origin in image coordinates
  const int hy0 = DIR == 0 ? oy0 : oy0 - 2, hx0 = DIR == 0 ? -2 : ox0;

  // halo staging in two halves of NA float4 per thread: slot (part, j) is the (pixel, channel
  // quad) pair (idx >> 3, idx & 7), idx = tid + 256·(2j + part).  Per slot the LDS float4 index and
  // the byte offset in the current source, WINO_OOB for a lane that reads zero (conv_wino.h: it
  // changes at most three times per launch and the main loop is cut there).
  int hoff[2][NA], hlds[2][NA];
  const int hq4 = 4 * (tid & 7);
  auto hoffsets = [&](int ss4, bool with_lds) {  // ss4: the source's pixel stride in bytes
#pragma unroll
    for (int part = 0; part < 2; ++part)
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        const int idx = tid + NTH * (2 * j + part);
        const int pix = idx >> 3;
        const int hr = pix / G::HC, hcol = pix - hr * G::HC;
        const int iy = hy0 + hr, ix = hx0 + hcol;
        const bool ok = idx < G::NH4 && iy >= 0 && iy < a.h && ix >= 0 && ix < W;
        const int p = (img * a.h + iy) * W + ix;
        hoff[part][j] = ok ? p * ss4 + hq4 * 4 : WINO_OOB;
        if (with_lds) hlds[part][j] = idx < G::NH4 ? G::addr(hr, hcol) + (idx & 7) : -1;
      }
  };
  floatx4 ra[NA];
  __amdgpu_buffer_rsrc_t hsrc;
  auto hsource = [&](int s) {  // stage s's source as a buffer from its first channel (scalar work)
    const bool s1 = s >= nst0;
    const float* src = s1 ? a.src1 : a.src0;
    const int cs = s1 ? a.c1 : a.c0;
    const int ss = s1 ? a.s1 : a.s0;
    const int cc = (s1 ? s - nst0 : s) * W5SC;
    hsrc = wino_rsrc(src + cc, (unsigned)(((long long)(npix - 1) * ss + cs - cc) * 4));
  };
  auto hfix = [&](int t) {  // the offsets for loading stage t, given stage t − 1's (conv_wino.h)
    const bool s1 = t >= nst0;
    if (t == nst0 && t > 0) hoffsets(a.s1 * 4, false);
    const int lim = s1 ? a.c1 - (t - nst0) * W5SC : a.c0 - t * W5SC;
    if (lim < W5SC) {
      const bool gone = hq4 >= lim;
#pragma unroll
      for (int part = 0; part < 2; ++part)
#pragma unroll
        for (int j = 0; j < NA; ++j) hoff[part][j] = gone ? WINO_OOB : hoff[part][j];
    }
  };
  auto hload = [&](int part) {
#pragma unroll
    for (int j = 0; j < NA; ++j) ra[j] = wino_bload(hsrc, hoff[part][j], 0);
  };
  auto hstore = [&](int buf, int part) {
#pragma unroll
    for (int j = 0; j < NA; ++j)
      if (G::NH4 % (2 * NTH) == 0 || hlds[part][j] >= 0) smem4[buf * G::BUF4 + hlds[part][j]] = ra[j];
  };

  // weights [nb32][sub-step (16 channels)][slot 8][q 2][lane 64][4]; slot 2·wave + x holds
  // point w5_point(wave, x)
  const int nsub = nst * W5NSUB;
  const __amdgpu_buffer_rsrc_t wsrc =
      wino_rsrc(a.weight + (size_t)by * NBW * nsub * 16 * 256, (unsigned)(NBW * nsub * 16 * 1024));
  floatx4 u[2][2][NBW];  // [q][x][nb]
  auto uload1 = [&](int t, int q) {
    const int tt = t < nsub ? t : nsub - 1;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int nb = 0; nb < NBW; ++nb)
        u[q][x][nb] = wino_bload(wsrc, lane * 16, ((((nb * nsub + tt) * 8 + 2 * wave + x) * 2 + q) * 1024));
  };

  // Bᵀ rows of this wave: waves 0-2 → V = b ± a (odd taps a = c1·d1 + c3·d3 + c5·d5, even taps
  // b = c2·d2 + c4·d4 + d6); wave 3 → V0 = (d6 − d0) + 5.25(d2 − d4), V7 = (d7 − d1) + 5.25(d3 − d5)
  const float c1 = wave == 0 ? 1.f : (wave == 1 ? 0.5f : 2.f);
  const float c3 = wave == 0 ? -4.25f : -2.5f;
  const float c5 = wave == 0 ? 1.f : (wave == 1 ? 2.f : 0.5f);
  const float c2 = wave == 0 ? 1.f : (wave == 1 ? 0.25f : 4.f);
  const float c4 = wave == 0 ? -4.25f : (wave == 1 ? -1.25f : -5.f);
  // the lane's tile: LDS float4 index of its input 0 along the conv axis (+ the channel half hh)
  const int tb = (DIR == 0 ? G::addr(li / G::TPR, 4 * (li % G::TPR)) : G::addr(0, li)) + hh;
  auto tapoff = [](int t) {  // LDS float4 offset of input t from input 0 (tiles start at c ≡ 0 mod 4)
    return DIR == 0 ? t * 8 + t / G::SK : t * G::ROWP;
  };
  // input transform of one 8-channel half q of sub-step k from LDS buffer buf: the taps this
  // wave needs (1..6, and 0, 7 for wave 3), then its two rows of Bᵀd
  auto vload = [&](int buf, int k, int q, floatx4(&d)[8], auto w3) {
    const floatx4* hb = smem4 + buf * G::BUF4 + tb + 4 * k + 2 * q;
#pragma unroll
    for (int t = 0; t < 8; ++t)
      if (decltype(w3)::value || (t > 0 && t < 7)) d[t] = hb[tapoff(t)];
  };
  auto vmath = [&](const floatx4(&d)[8], floatx4(&v)[2], auto w3) {
    if constexpr (!decltype(w3)::value) {
      const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
      const floatx4 av = fma_s4(d[5], c5, fma_s4(d[3], c3, fma_s4(d[1], c1, zero)));
      const floatx4 bv = fma_s4(d[4], c4, fma_s4(d[2], c2, d[6]));
      v[0] = add4(bv, av);
      v[1] = sub4(bv, av);
    } else {
      v[0] = fma_s4(sub4(d[2], d[4]), 5.25f, sub4(d[6], d[0]));
      v[1] = fma_s4(sub4(d[3], d[5]), 5.25f, sub4(d[7], d[1]));
    }
  };

  floatx16 acc[2][NBW];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[x][nb][e] = 0.f;

  // the MFMAs of 8-channel half q, then its weights for sub-step tnext
  auto half = [&](const floatx4(&v)[2][2], int q, int tnext) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb)
          acc[x][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[q][x][e], u[q][x][nb][e], acc[x][nb], 0, 0, 0);
    uload1(tnext, q);
#if WINO_SCHED_BARRIER
    __builtin_amdgcn_sched_barrier(0);  // the reload stays a half sub-step ahead (conv_wino.h)
#endif
  };

  // The main loop is instantiated per transform shape (waves 0-2 / wave 3; the wave index is
  // uniform), so its body has no branches and the next sub-step's transform can be woven
  // between this sub-step's MFMAs in program order (the compiler issues in order: the LDS
  // latency and the VALU then sit under the MFMAs instead of in front of them).
  auto mainloop = [&](auto w3) {
    floatx4 d[8];
    uload1(0, 0);
    uload1(0, 1);
    hoffsets((nst0 ? a.s0 : a.s1) * 4, true);
    hfix(0);
    hsource(0);
    hload(0);
    hstore(0, 0);
    hload(1);
    hstore(0, 1);
    __builtin_amdgcn_s_waitcnt(0);  // see conv_wino.h: keeps the prefetch off the MFMAs' wait
    __syncthreads();
    wino_stamp(P.stamps, 1);
    floatx4 vA[2][2], vB[2][2];
    vload(0, 0, 0, d, w3);
    vmath(d, vA[0], w3);
    vload(0, 0, 1, d, w3);
    vmath(d, vA[1], w3);
    // the stage loop, cut where the offsets change: hfix outside the inner loop (conv_wino.h)
    for (int s = 0; s < nst;) {
      const int t = s + 1 < nst ? s + 1 : s;
      hfix(t);
      const int b = wino_next_change(t, nst0, nst, a.c0, a.c1, W5SC);
      const int send = b < nst ? b - 1 : nst;
      for (; s < send; ++s) {
        wino_prio(s, nst);
        const int buf = s & 1;
        const int t0 = s * W5NSUB;
        hsource(s + 1 < nst ? s + 1 : s);  // the last stage re-stages itself (no branches)
        hload(0);
        vload(buf, 1, 0, d, w3);
        half(vA, 0, t0 + 1);
        vmath(d, vB[0], w3);
        vload(buf, 1, 1, d, w3);
        half(vA, 1, t0 + 1);
        vmath(d, vB[1], w3);
        hstore(buf ^ 1, 0);
        hload(1);
        half(vB, 0, t0 + 2);
        half(vB, 1, t0 + 2);
        hstore(buf ^ 1, 1);
        __syncthreads();
        vload(buf ^ 1, 0, 0, d, w3);
        vmath(d, vA[0], w3);
        vload(buf ^ 1, 0, 1, d, w3);
        vmath(d, vA[1], w3);
      }
    }
  };
  if (wave == 3)
    mainloop(std::true_type{});
  else
    mainloop(std::false_type{});
#if WINO_PRIO
  __builtin_amdgcn_s_setprio(0);
#endif

#ifdef WX_NO_EPI
  {
    float t = 0.f;
    for (int x = 0; x < 2; ++x)
      for (int nb = 0; nb < NBW; ++nb)
        for (int e = 0; e < 16; ++e) t += acc[x][nb][e];
    if (t == 12345.678f) a.out[tid] = t;
    return;
  }
#endif
  // epilogue: M[ξ][co][tile] in LDS (tiles contiguous, WEP-float rows: a lane's accumulator
  // rows r..r+3 are 4 consecutive tiles → one 16-B store; conflict-free for the b128 stores and
  // loads, see conv_wino.h), then every thread takes a run of NT tiles of its channel, 4 tiles
  // per 16-B load of each point, and y[o] = Σ_ξ Aᵀ[o][ξ]·M[ξ].
  // Every global read of the epilogue (bias map, h, z) is issued first — before the points'
  // LDS exchange, so its latency runs under the exchange and the output transform instead of
  // after them (in a one-round grid every workgroup reaches its epilogue at once) — and before
  // any store (the stores may alias them as far as the compiler knows).
  constexpr int WEP = W5TM + 4;
  const int co = tid % BNW;
  const int col = by * BNW + co;
  const bool col_ok = col < a.cout;
  constexpr int GROUPS = NTH / BNW;
  constexpr int NT = W5TM / GROUPS;  // tiles per thread
  static_assert(NT % 4 == 0, "epilogue: whole 16-B tile loads per thread");
  const int mbase = (tid / BNW) * NT;
  int pix[NT][4];  // output pixel (n·h·w < 2^31)
#pragma unroll
  for (int k = 0; k < NT; ++k)
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int m = mbase + k;
      const int oy = DIR == 0 ? oy0 + m / G::TPR : oy0 + o;
      const int ox = DIR == 0 ? 4 * (m % G::TPR) + o : ox0 + m;
      pix[k][o] = (img * a.h + oy) * W + ox;
    }
  const int hcn = a.cout >> 1;
  const bool zr_h = EPI == SCFLOW_EPI_GRU_ZR && col >= hcn;  // the r·h half of z|r
  float bm[NT][4], hv[NT][4], zv[NT][4];
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const size_t p0 = (size_t)pix[k][0];
    constexpr int OS = DIR == 0 ? 1 : W;  // pixels between a tile's outputs
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      bm[k][o] = col_ok && a.bias_map ? a.bias_map[p0 * a.sbm + col + o * OS * a.sbm] : 0.f;
      hv[k][o] = 0.f;
      zv[k][o] = 0.f;
      if constexpr (EPI == SCFLOW_EPI_GRU_ZR) {
        if (col_ok && zr_h) hv[k][o] = a.hid[p0 * a.sh + (col - hcn) + o * OS * a.sh];
      } else if constexpr (EPI == SCFLOW_EPI_GRU_Q) {
        if (col_ok) {
          zv[k][o] = a.gate[p0 * a.sg + col + o * OS * a.sg];
          hv[k][o] = a.hid[p0 * a.sh + col + o * OS * a.sh];
        }
      }
    }
  }
  __syncthreads();
  wino_stamp(P.stamps, 2);
  float* S = smem;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        floatx4 v;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) v[rr] = acc[x][nb][4 * q4 + rr];
        *(floatx4*)&S[(w5_point(wave, x) * BNW + nb * 32 + li) * WEP + 8 * q4 + 4 * hh] = v;
      }
  __syncthreads();
  if (!col_ok) return;
  const float bias = a.bias ? a.bias[col] : 0.f;
  float y[NT][4];
#pragma unroll
  for (int k4 = 0; k4 < NT / 4; ++k4) {
    floatx4 mv[8];
#pragma unroll
    for (int xi = 0; xi < 8; ++xi) mv[xi] = *(const floatx4*)&S[(xi * BNW + co) * WEP + mbase + 4 * k4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * k4 + e;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        float v = 0.f;
#pragma unroll
        for (int xi = 0; xi < 8; ++xi)
          if (kW5AT[o][xi] != 0.f) v += kW5AT[o][xi] * mv[xi][e];
        y[k][o] = v + bias + bm[k][o];
      }
    }
  }
  // a tile's 4 outputs are OSTEP pixels apart: one 64-bit base per tile, 32-bit offsets
  constexpr int OSTEP = DIR == 0 ? 1 : W;
  if constexpr (EPI == SCFLOW_EPI_PLAIN) {
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      float* ob = a.out + (size_t)pix[k][0] * a.so + col;
#pragma unroll
      for (int o = 0; o < 4; ++o) ob[o * OSTEP * a.so] = act_apply(y[k][o], a.act);
    }
  } else if constexpr (EPI == SCFLOW_EPI_GRU_ZR) {
    if (!zr_h) {
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        float* gb = a.gate + (size_t)pix[k][0] * a.sg + col;
#pragma unroll
        for (int o = 0; o < 4; ++o) gb[o * OSTEP * a.sg] = sigmoidf_(y[k][o]);
      }
    } else {
      const int c = col - hcn;
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        float* rb = a.rh + (size_t)pix[k][0] * a.srh + c;
#pragma unroll
        for (int o = 0; o < 4; ++o) rb[o * OSTEP * a.srh] = sigmoidf_(y[k][o]) * hv[k][o];
      }
    }
  } else {  // GRU_Q
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      float* hb = a.hid + (size_t)pix[k][0] * a.sh + col;
#pragma unroll
      for (int o = 0; o < 4; ++o)
        hb[o * OSTEP * a.sh] = (1.f - zv[k][o]) * hv[k][o] + zv[k][o] * tanhf_(y[k][o]);
    }
  }
  if (P.stamps) {
    __builtin_amdgcn_s_waitcnt(0);
    wino_stamp(P.stamps, 3);
  }
}

// U_ξ = Σ_j G[ξ][j]·g[j] (fp64) per (co, ci), packed [nb32][sub-step][slot][q][lane][4] with
// lane = li + 32·hh ↔ co = 32·nb32 + li, padded channel kc = 16·sub-step + 8·q + 4·hh + e.
__global__ void wino5_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int cout,
                                  int c0, int c1, int cp0, int nst, long long total) {
  const double Gm[8][5] = {{-1.0, 0.0, 0.0, 0.0, 0.0},
                           {-2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9},
                           {-2.0 / 9, 2.0 / 9, -2.0 / 9, 2.0 / 9, -2.0 / 9},
                           {1.0 / 90, 1.0 / 45, 2.0 / 45, 4.0 / 45, 8.0 / 45},
                           {1.0 / 90, -1.0 / 45, 2.0 / 45, -4.0 / 45, 8.0 / 45},
                           {32.0 / 45, 16.0 / 45, 8.0 / 45, 4.0 / 45, 2.0 / 45},
                           {32.0 / 45, -16.0 / 45, 8.0 / 45, -4.0 / 45, 2.0 / 45},
                           {0.0, 0.0, 0.0, 0.0, 1.0}};
  const int cin = c0 + c1;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    long long r = idx;
    const int e = (int)(r & 3); r >>= 2;
    const int lane = (int)(r & 63); r >>= 6;
    const int q = (int)(r & 1); r >>= 1;
    const int slot = (int)(r & 7); r >>= 3;
    const int xi = w5_point(slot >> 1, slot & 1);
    const int s = (int)(r % nst);
    const int nb = (int)(r / nst);
    const int o = nb * 32 + (lane & 31);
    const int kc = s * W5KC + 8 * q + 4 * (lane >> 5) + e;
    int ci = -1;
    if (kc < cp0) {
      if (kc < c0) ci = kc;
    } else if (kc - cp0 < c1) {
      ci = c0 + (kc - cp0);
    }
    float v = 0.f;
    if (o < cout && ci >= 0) {
      const float* g = w + ((size_t)o * cin + ci) * 5;
      double acc = 0.0;
      for (int j = 0; j < 5; ++j) acc += Gm[xi][j] * (double)g[j];
      v = (float)acc;
    }
    out[idx] = v;
  }
}
