// What the bf16 MFMA direct convs share — conv_sep_bf16.h (1×5 / 5×1, SCFLOW_CONV_BF16) and
// conv3_bf16.h (3×3, SCFLOW_CONV_BF16_3X3 / _3X3N): the vector types and stage constants, the
// fp32 → bf16 rounding, the halo stager, the packed-weight addressing and its pack kernel, and the
// 32×32 MFMA block's C/D row map.  Included once by conv.hip (inside its anonymous namespace),
// before the two kernel headers.  The K loops (weight prefetch depth) and the epilogues are the
// kernels' own.

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx8 __attribute__((ext_vector_type(8)));

constexpr int SBSC = 32;    // input channels per stage
constexpr int SBKC = 16;    // input channels per MFMA k-step
constexpr int SBPITCH = 5;  // 16-B slots per halo pixel: 4 of channels + 1 pad

// 8 fp32 → 8 bf16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ floatx4 bf16_round8(floatx4 lo, floatx4 hi) {
  const floatx8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(floatx4, __builtin_convertvector(v, bf16x8));
}

// fp32 bits → bf16 bits, round to nearest even (finite weights)
__device__ __forceinline__ unsigned bf16_bits(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// The halo stager of a 256-thread workgroup: one stage is 32 channels of one source over a halo
// of HR rows × HC columns, held in LDS as [HR·HC pixels][SBPITCH] 16-B slots of 8 bf16, double-
// buffered.  Slot idx = tid + 256·j (j < NA) is (pixel idx >> 2, channels 8·(idx & 3) .. + 7): a
// thread stages the same 8 channels of each of its pixels.  A stage goes through the staging
// registers ra: load() issues the buffer loads (pixels outside the image read as 0), store()
// rounds them to bf16 into one LDS buffer; what a kernel does to ra in between is its own.
template <int HR, int HC>
struct Bf16Halo {
  static constexpr int NH = HR * HC * 4;            // 8-channel slots of one stage's halo
  static constexpr int NA = (NH + 255) / 256;       // slots per thread
  static constexpr int BUF = HR * HC * SBPITCH;     // 16-B LDS slots of one buffer
  static constexpr size_t LDS_BYTES = (size_t)2 * BUF * 16;

  // pixel index (img, iy, ix) of each of this thread's slots in an h × w image, halo origin
  // (hy0, hx0); −1 outside the image (the neighbouring sample's rows included) or past NH
  static __device__ __forceinline__ void pixels(int (&hpix)[NA], int tid, int img, int h, int w,
                                                int hy0, int hx0) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int idx = tid + 256 * j;
      const int pix = idx >> 2;
      const int hr = pix / HC, hcol = pix - hr * HC;
      const int iy = hy0 + hr, ix = hx0 + hcol;
      const bool ok = idx < NH && iy >= 0 && iy < h && ix >= 0 && ix < w;
      hpix[j] = ok ? (img * h + iy) * w + ix : -1;
    }
  }
  // stage s (source 0's nst0 stages, then source 1's) of a's npix pixels into ra
  static __device__ __forceinline__ void load(floatx4 (&ra)[NA][2], const int (&hpix)[NA], int tid,
                                              const scflow_conv_args& a, int nst0, int npix, int s) {
    const int hq = tid & 3;
    const bool s1 = s >= nst0;
    const float* src = s1 ? a.src1 : a.src0;
    const int cs = s1 ? a.c1 : a.c0;
    const int ss = s1 ? a.s1 : a.s0;
    const int cc = (s1 ? s - nst0 : s) * SBSC;
    const __amdgpu_buffer_rsrc_t hsrc =
        wino_rsrc(src + cc, (unsigned)(((long long)(npix - 1) * ss + cs - cc) * 4));
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int p = hpix[j];
      const int off = p >= 0 ? p * ss * 4 + hq * 32 : WINO_OOB;
      ra[j][0] = wino_bload(hsrc, off, 0);
      ra[j][1] = wino_bload(hsrc, p >= 0 ? off + 16 : WINO_OOB, 0);
    }
  }
  // ra, rounded to bf16, into the LDS buffer at buf
  static __device__ __forceinline__ void store(floatx4* buf, const floatx4 (&ra)[NA][2], int tid) {
    const int hq = tid & 3;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int idx = tid + 256 * j;
      if (NH % 256 == 0 || idx < NH) buf[(idx >> 2) * SBPITCH + hq] = bf16_round8(ra[j][0], ra[j][1]);
    }
  }
};

// Packed weights: bf16 in B-fragment lane order, [nb32][k-step][tap][lane][8 bf16] — 1 KiB per
// (32 output channels, 16-channel k-step, tap); lane li + 32·hh holds output channel 32·nb32 + li,
// input channels 16·k-step + 8·hh + 0..7.  The byte offset of block (nb, ks, tap) of nks k-steps
// of TAPS taps.  The 3×3 kernel's ring walks groups g = 3·ks + ty of one tap row: its
// bf16_wblock<3>(nb, 3·nks, g, tx) is this layout's bf16_wblock<9>(nb, nks, ks, 3·ty + tx).
template <int TAPS>
__device__ __forceinline__ int bf16_wblock(int nb, int nks, int ks, int tap) {
  return ((nb * nks + ks) * TAPS + tap) * 1024;
}

// Row of accumulator element r (0..15) of lane half hh in the 32×32 MFMA block's C/D layout
// (col = lane & 31) — the direct conv's (conv_mfma_kernel)
__device__ __forceinline__ int mfma32_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// OIHW fp32 (taps = kh·kw, tap = kw·ky + kx) → the packed layout above, two bf16 per packed float
// (element 2i in the low half).  Source 1's channels follow source 0's directly (both are
// multiples of 32); output channels past cout in the padded blocks are 0.
__global__ void bf16_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int cout,
                                 int cin, int nks, int taps, long long total) {
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    long long r = idx;
    const int e2 = (int)(r & 3); r >>= 2;
    const int lane = (int)(r & 63); r >>= 6;
    const int tap = (int)(r % taps); r /= taps;
    const int ks = (int)(r % nks);
    const int nb = (int)(r / nks);
    const int o = nb * 32 + (lane & 31);
    const int ci = ks * SBKC + 8 * (lane >> 5) + 2 * e2;
    unsigned bits = 0;
    if (o < cout) {
      const float* g = w + ((size_t)o * cin + ci) * taps + tap;
      bits = bf16_bits(g[0]) | (bf16_bits(g[taps]) << 16);
    }
    out[idx] = __builtin_bit_cast(float, bits);
  }
}
