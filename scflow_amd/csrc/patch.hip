// Patches from full frames: the reference's test-time formatting
// ComputeBbox → Crop → Resize → Pad → RemapPose(adapt_intrinsic) → Normalize
// (datasets/pipelines/geometry_transform.py:155-500, formatting.py:42-91) as two launches that
// read their geometry from device memory, so neither needs the host to know a crop's size.
//
//   patch_boxes_kernel    one workgroup per object: project the model points, min/max by a wave
//                         reduction then LDS, thread 0 derives the crop geometry, T and k.
//   patch_extract_kernel  one launch for all patches: a workgroup owns a band of output rows of
//                         one patch, a thread four neighbouring output pixels of every channel
//                         plane (one 16-byte store per plane, 1 KiB per wave).  The taps are read
//                         directly; with SCFLOW_PATCH_LDS the two source rows of each output row
//                         are staged in LDS with aligned dword loads where the crop row fits the
//                         budget.  Both routes do the same arithmetic on the same values.
//
// Every fp32 expression here is part of the contract (tests/patch_restatement.py restates it
// operation by operation), so contraction into FMAs is off for the whole file.
#include "patch_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int PB_THREADS = 256;
constexpr int PX_LDS_BYTES = 32 * 1024;  // staging budget of one workgroup
constexpr int PX_MAX_SLOTS = 64;         // two source rows per output row, ≤ 32 rows per band

// 0: every tap is read from global memory (the measured-faster route at the sizes timed,
// DESIGN.md §15); other: source rows staged in LDS where the crop row fits the budget
EnvSwitch g_patch_lds("SCFLOW_PATCH_LDS", 0);

// output rows per workgroup: 1024 output pixels (256 threads × 4), at most the whole patch
__host__ __device__ inline int px_rows(int S) {
  int r = 1024 / S;
  if (r < 1) r = 1;
  return r > S ? S : r;
}

// bytes of one staged source row: the crop row plus up to 3 bytes in front of it (the row is
// loaded from the 4-byte boundary below its first byte), rounded up to 16
__host__ __device__ inline int px_row_bytes(int cw, int bpp) { return (cw * bpp + 3 + 15) & ~15; }

__host__ __device__ inline bool px_staged(int cw, int bpp, int S) {
  return cw >= 1 && cw <= PX_MAX_CROP &&
         2ll * px_rows(S) * px_row_bytes(cw, bpp) <= (long long)PX_LDS_BYTES;
}

struct PatchBoxArgs {
  const float* points;
  const int* counts;
  const int* labels;
  const float* R;
  const float* t;
  const float* ori_k;
  const int* frame_index;
  const float* ratio;
  float* bbox;
  int* geom;
  float* T;
  float* k;
  unsigned char* valid;
  int num_classes, max_points, k_per_frame, num_frames, H, W, S;
};

__global__ __launch_bounds__(PB_THREADS) void patch_boxes_kernel(PatchBoxArgs a) {
  __shared__ float red[4][PB_THREADS / 64];
  __shared__ int red_bad[PB_THREADS / 64];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int label = a.labels[i];
  const int fi = a.frame_index ? a.frame_index[i] : 0;
  const bool frame_ok = !a.frame_index || (fi >= 0 && fi < a.num_frames);
  int cnt = 0;
  if (label >= 0 && label < a.num_classes) {
    cnt = a.counts[label];
    cnt = cnt < 0 ? 0 : (cnt > a.max_points ? a.max_points : cnt);
  }
  float K[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (!a.k_per_frame || frame_ok) {
    const float* kp = a.ori_k + 9 * (size_t)(a.k_per_frame ? fi : i);
    for (int j = 0; j < 9; ++j) K[j] = kp[j];
  }
  float R[9], t[3];
  for (int j = 0; j < 9; ++j) R[j] = a.R[9 * (size_t)i + j];
  for (int j = 0; j < 3; ++j) t[j] = a.t[3 * (size_t)i + j];

  float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
  int bad = 0;
  const float* pts = a.points + (size_t)(cnt ? label : 0) * a.max_points * 3;
  for (int p = tid; p < cnt; p += PB_THREADS) {
    const float X = pts[3 * p], Y = pts[3 * p + 1], Z = pts[3 * p + 2];
    float c[3], q[3];
    for (int r = 0; r < 3; ++r) c[r] = ((R[3 * r] * X + R[3 * r + 1] * Y) + R[3 * r + 2] * Z) + t[r];
    for (int r = 0; r < 3; ++r) q[r] = (K[3 * r] * c[0] + K[3 * r + 1] * c[1]) + K[3 * r + 2] * c[2];
    bad |= !(q[2] > 0.f);
    const float x = q[0] / q[2], y = q[1] / q[2];
    lo_x = fminf(lo_x, x), hi_x = fmaxf(hi_x, x);
    lo_y = fminf(lo_y, y), hi_y = fmaxf(hi_y, y);
    bad |= !(isfinite(x) && isfinite(y));  // fminf / fmaxf would drop a NaN
  }
  for (int off = 32; off; off >>= 1) {
    lo_x = fminf(lo_x, __shfl_xor(lo_x, off)), hi_x = fmaxf(hi_x, __shfl_xor(hi_x, off));
    lo_y = fminf(lo_y, __shfl_xor(lo_y, off)), hi_y = fmaxf(hi_y, __shfl_xor(hi_y, off));
    bad |= __shfl_xor(bad, off);
  }
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    red[0][w] = lo_x, red[1][w] = lo_y, red[2][w] = hi_x, red[3][w] = hi_y, red_bad[w] = bad;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < PB_THREADS / 64; ++w) {
    lo_x = fminf(lo_x, red[0][w]), lo_y = fminf(lo_y, red[1][w]);
    hi_x = fmaxf(hi_x, red[2][w]), hi_y = fmaxf(hi_y, red[3][w]);
    bad |= red_bad[w];
  }
  const float l = lo_x, tp = lo_y, r = hi_x, b = hi_y;
  float* bb = a.bbox + 4 * (size_t)i;
  bb[0] = l, bb[1] = tp, bb[2] = r, bb[3] = b;

  bool ok = !bad && frame_ok && isfinite(l) && isfinite(tp) && isfinite(r) && isfinite(b);
  const float side = fmaxf(r - l, b - tp);
  const float xc = (l + r) / 2.f, yc = (tp + b) / 2.f;
  const float sr = side * a.ratio[i];
  const float half = sr / 2.f;
  ok = ok && isfinite(sr) && !(sr < 1.f);
  const float e[4] = {xc - half, yc - half, xc + half, yc + half};
  for (int j = 0; j < 4; ++j) ok = ok && fabsf(e[j]) < (float)PX_MAX_ORIGIN;
  int g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float T[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, k[9];
  for (int j = 0; j < 9; ++j) k[j] = K[j];
  if (ok) {
    const int x1 = (int)e[0], y1 = (int)e[1], x2 = (int)e[2], y2 = (int)e[3];  // toward zero
    const int cw = x2 - x1 + 1, ch = y2 - y1 + 1, m = cw > ch ? cw : ch;
    ok = m <= SCFLOW_PATCH_MAX_CROP && x2 >= 0 && y2 >= 0 && x1 <= a.W - 1 && y1 <= a.H - 1;
    if (ok) {
      const int S = a.S;
      const float sf = (float)S / (float)m;
      const int nw = (2 * cw * S + m) / (2 * m), nh = (2 * ch * S + m) / (2 * m);
      const int left = (S - nw) / 2, top = (S - nh) / 2;
      g[0] = x1, g[1] = y1, g[2] = x2, g[3] = y2, g[4] = nw, g[5] = nh, g[6] = left, g[7] = top;
      const float Tc[9] = {1.f, 0.f, -(float)x1, 0.f, 1.f, -(float)y1, 0.f, 0.f, 1.f};
      const float Ts[9] = {sf, 0.f, 0.f, 0.f, sf, 0.f, 0.f, 0.f, 1.f};
      const float Tp[9] = {1.f, 0.f, (float)left, 0.f, 1.f, (float)top, 0.f, 0.f, 1.f};
      float ps[9];
      mat3_mul(Tp, Ts, ps);
      mat3_mul(ps, Tc, T);
      mat3_mul(T, K, k);
    }
  }
  for (int j = 0; j < 8; ++j) a.geom[8 * (size_t)i + j] = g[j];
  for (int j = 0; j < 9; ++j) a.T[9 * (size_t)i + j] = T[j], a.k[9 * (size_t)i + j] = k[j];
  a.valid[i] = ok ? 1 : 0;
}

struct PatchExtractArgs {
  const void* frames;
  const int* frame_index;
  const int* geom;
  const unsigned char* valid;
  float* out;
  int F, H, W, S;
  float pad;
  float mean[3], std[3];
  int to_rgb, quantize, nearest, use_lds;
};

template <typename T, int C>
__global__ __launch_bounds__(PX_THREADS) void patch_extract_kernel(PatchExtractArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // PX_LDS_BYTES with use_lds
  __shared__ unsigned long long slot_a0[PX_MAX_SLOTS], slot_a1[PX_MAX_SLOTS];
  constexpr int BPP = C * (int)sizeof(T);
  const int S = a.S, rows = px_rows(S), bands = (S + rows - 1) / rows;
  const int obj = blockIdx.x / bands, row0 = (blockIdx.x % bands) * rows, tid = threadIdx.x;
  const int nrows = row0 + rows <= S ? rows : S - row0;

  const int* gp = a.geom + 8 * (size_t)obj;
  const int x1 = gp[0], y1 = gp[1], x2 = gp[2], y2 = gp[3];
  const int nw = gp[4], nh = gp[5], left = gp[6], top = gp[7];
  const int fi = a.frame_index[obj];
  // the geometry comes from device memory: anything that is not a patch geometry is treated as
  // an invalid object, so no index below leaves the frame, the patch or 32 bits
  const bool ok = a.valid[obj] != 0 && fi >= 0 && fi < a.F && x1 >= -PX_MAX_ORIGIN &&
                  x1 <= PX_MAX_ORIGIN && y1 >= -PX_MAX_ORIGIN && y1 <= PX_MAX_ORIGIN && x2 >= x1 &&
                  y2 >= y1 && x2 - x1 < PX_MAX_CROP && y2 - y1 < PX_MAX_CROP && nw >= 1 &&
                  nh >= 1 && left >= 0 && top >= 0 && nw <= S - left && nh <= S - top;
  const int cw = ok ? x2 - x1 + 1 : 1, ch = ok ? y2 - y1 + 1 : 1;
  const T* frame = (const T*)a.frames + (size_t)(ok ? fi : 0) * a.H * a.W * C;

  const bool staged = ok && a.use_lds && !a.nearest && px_staged(cw, BPP, S);  // block-uniform
  const int rb = px_row_bytes(cw, BPP);
  const int ca = x1 > 0 ? x1 : 0, cb = x2 < a.W - 1 ? x2 : a.W - 1;  // the crop's columns in the frame
  if (staged) {
    if (tid < 2 * nrows) {
      unsigned long long a0 = 0, a1 = 0;
      const int oy = row0 + (tid >> 1) - top;
      if (oy >= 0 && oy < nh && ca <= cb) {
        int y0;
        float fy;
        linear_coord(oy, ch, nh, y0, fy);
        int ys = y0 + (tid & 1);
        ys = ys < ch - 1 ? ys : ch - 1;
        const int fy_ = y1 + ys;
        if (fy_ >= 0 && fy_ < a.H) {
          const unsigned char* rowp = (const unsigned char*)(frame + ((size_t)fy_ * a.W) * C);
          a0 = (unsigned long long)(uintptr_t)(rowp + (size_t)ca * BPP);
          a1 = (unsigned long long)(uintptr_t)(rowp + (size_t)(cb + 1) * BPP);
        }
      }
      slot_a0[tid] = a0, slot_a1[tid] = a1;
    }
    __syncthreads();
    // every byte of [a0, a1) lies in the frame; whole dwords inside it are loaded as dwords
    const int dw = rb / 4;
    for (int idx = tid; idx < 2 * nrows * dw; idx += PX_THREADS) {
      const int slot = idx / dw, d = idx - slot * dw;
      const unsigned long long a0 = slot_a0[slot], a1 = slot_a1[slot];
      const unsigned long long lo = (a0 & ~3ull) + 4ull * d;
      if (lo >= a1) continue;
      unsigned char* dst = lds + (size_t)slot * rb + 4 * d;
      if (lo >= a0 && lo + 4 <= a1) {
        *(uint32_t*)dst = *(const uint32_t*)(uintptr_t)lo;
      } else {
        for (int k = 0; k < 4; ++k)
          if (lo + k >= a0 && lo + k < a1) dst[k] = *(const unsigned char*)(uintptr_t)(lo + k);
      }
    }
    __syncthreads();
  }

  const int quads = S / 4;
  for (int item = tid; item < nrows * quads; item += PX_THREADS) {
    const int rr = item / quads, q = item - rr * quads;
    const int dy = row0 + rr, oy = dy - top;
    const bool row_in = ok && oy >= 0 && oy < nh;
    int y0 = 0, ya = 0, yb = 0;
    float fy = 0.f;
    if (row_in) {
      if (a.nearest) {
        y0 = (int)(((long long)oy * ch) / nh);
        ya = yb = y0 < ch - 1 ? y0 : ch - 1;
      } else {
        linear_coord(oy, ch, nh, y0, fy);
        ya = y0, yb = y0 + 1 < ch - 1 ? y0 + 1 : ch - 1;
      }
    }
    const int fya = y1 + ya, fyb = y1 + yb;  // frame rows of the two taps
    const bool ina = fya >= 0 && fya < a.H, inb = fyb >= 0 && fyb < a.H;
    // Per pixel: the two source columns and fx.  A tap that names no frame pixel gets the offset
    // of one that does (column 0 of the row read), so every load below is unconditional and in
    // bounds and the loads of all four pixels are in flight together; the selects after them
    // put the pad value in its place.
    const int col0 = staged ? ca : 0;  // first frame column of the row read
    int offa[4], offb[4];
    float fx[4];
    bool pin[4], jna[4], jnb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ox = 4 * q + e - left;
      pin[e] = row_in && ox >= 0 && ox < nw;
      int x0, xa = 0, xb = 0;
      fx[e] = 0.f;
      if (pin[e]) {
        if (a.nearest) {
          x0 = (int)(((long long)ox * cw) / nw);
          xa = xb = x0 < cw - 1 ? x0 : cw - 1;
        } else {
          linear_coord(ox, cw, nw, x0, fx[e]);
          xa = x0, xb = x0 + 1 < cw - 1 ? x0 + 1 : cw - 1;
        }
      }
      const int fxa = x1 + xa, fxb = x1 + xb;
      jna[e] = pin[e] && fxa >= 0 && fxa < a.W, jnb[e] = pin[e] && fxb >= 0 && fxb < a.W;
      offa[e] = ((jna[e] ? fxa : col0) - col0) * BPP, offb[e] = ((jnb[e] ? fxb : col0) - col0) * BPP;
    }
    T raw[4][4][C];  // [pixel][tap a, b, c, d][source channel]
#define PX_LOAD_TAPS(ROW_A, ROW_B)                                              \
  _Pragma("unroll") for (int e = 0; e < 4; ++e)                                 \
    _Pragma("unroll") for (int c = 0; c < C; ++c) {                             \
      raw[e][0][c] = *(const T*)((ROW_A) + offa[e] + c * (int)sizeof(T));       \
      raw[e][1][c] = *(const T*)((ROW_A) + offb[e] + c * (int)sizeof(T));       \
      raw[e][2][c] = *(const T*)((ROW_B) + offa[e] + c * (int)sizeof(T));       \
      raw[e][3][c] = *(const T*)((ROW_B) + offb[e] + c * (int)sizeof(T));       \
    }
    if (staged) {  // an unstaged slot (row outside the frame) holds nothing that is used
      const unsigned char* la = lds + (size_t)(2 * rr) * rb + (int)(slot_a0[2 * rr] & 3);
      const unsigned char* lb = lds + (size_t)(2 * rr + 1) * rb + (int)(slot_a0[2 * rr + 1] & 3);
      PX_LOAD_TAPS(la, lb)
    } else {
      const unsigned char* ga = (const unsigned char*)(frame + (size_t)(ina ? fya : 0) * a.W * C);
      const unsigned char* gb = (const unsigned char*)(frame + (size_t)(inb ? fyb : 0) * a.W * C);
      PX_LOAD_TAPS(ga, gb)
    }
#undef PX_LOAD_TAPS

    float v[C][4];
    const float gy = 1.f - fy;
#pragma unroll
    for (int co = 0; co < C; ++co) {
      const float padn = (a.pad - a.mean[co]) / a.std[co];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in = ((k & 2) ? inb : ina) && ((k & 1) ? jnb[e] : jna[e]);
          const float r = (float)(a.to_rgb ? raw[e][k][C - 1 - co] : raw[e][k][co]);
          p[k] = in ? r : a.pad;
        }
        float val = p[0];
        if (!a.nearest) {
          const float gx = 1.f - fx[e];
          const float up = gx * p[0] + fx[e] * p[1], dn = gx * p[2] + fx[e] * p[3];
          val = gy * up + fy * dn;
          if (a.quantize) val = rintf(val);
        }
        v[co][e] = pin[e] ? (val - a.mean[co]) / a.std[co] : padn;
      }
    }
    for (int co = 0; co < C; ++co) {
      float* o = a.out + (((size_t)obj * C + co) * S + dy) * S + 4 * q;
      *(floatx4*)o = floatx4{v[co][0], v[co][1], v[co][2], v[co][3]};
    }
  }
}

}  // namespace

SCFLOW_API int scflow_patch_staged(int cw, int channels, int dtype, int size) {
  if (cw < 1 || size < 4 || size > 4096 || size % 4) return SCFLOW_EINVAL;
  const bool u8 = dtype == SCFLOW_PATCH_U8;
  if (!((u8 && (channels == 1 || channels == 3)) || (dtype == SCFLOW_PATCH_F32 && channels == 1)))
    return SCFLOW_EUNSUPPORTED;
  return g_patch_lds.get() != 0 && px_staged(cw, channels * (u8 ? 1 : 4), size) ? 1 : 0;
}

SCFLOW_API int scflow_patch_boxes(const float* points, const int* counts, const int* labels,
                                  const float* R, const float* t, const float* ori_k,
                                  const int* frame_index, const float* ratio, float* bbox, int* geom,
                                  float* T, float* k, unsigned char* valid, int n, int num_classes,
                                  int max_points, int k_per_frame, int num_frames, int height,
                                  int width, int size, void* stream) {
  if (!points || !counts || !labels || !R || !t || !ori_k || !ratio || !bbox || !geom || !T || !k ||
      !valid || n <= 0 || num_classes <= 0 || max_points <= 0 || height <= 0 || width <= 0 ||
      (k_per_frame && !frame_index) || (frame_index && num_frames <= 0))
    return SCFLOW_EINVAL;
  if (size < 4 || size > 4096 || size % 4 || height > PX_MAX_ORIGIN || width > PX_MAX_ORIGIN ||
      (long long)num_classes * max_points > (1ll << 28))
    return SCFLOW_EUNSUPPORTED;
  PatchBoxArgs a{points, counts, labels, R, t, ori_k, frame_index, ratio, bbox, geom, T, k, valid,
                 num_classes, max_points, k_per_frame ? 1 : 0, num_frames, height, width, size};
  hipLaunchKernelGGL(patch_boxes_kernel, dim3(n), dim3(PB_THREADS), 0, (hipStream_t)stream, a);
  return scflow_launch_status();
}

SCFLOW_API int scflow_patch_extract(const void* frames, const int* frame_index, const int* geom,
                                    const unsigned char* valid, float* out, int n, int num_frames,
                                    int height, int width, int channels, int dtype, int size,
                                    float pad, const float* mean, const float* std, int flags,
                                    void* stream) {
  if (!frames || !frame_index || !geom || !valid || !out || n <= 0 || num_frames <= 0 ||
      height <= 0 || width <= 0 || (flags & ~7))
    return SCFLOW_EINVAL;
  const bool u8 = dtype == SCFLOW_PATCH_U8;
  if (!((u8 && (channels == 1 || channels == 3)) || (dtype == SCFLOW_PATCH_F32 && channels == 1)))
    return SCFLOW_EUNSUPPORTED;
  if (size < 4 || size > 4096 || size % 4 || height > PX_MAX_ORIGIN || width > PX_MAX_ORIGIN)
    return SCFLOW_EUNSUPPORTED;
  const int rows = px_rows(size), bands = (size + rows - 1) / rows;
  if ((long long)n * bands >= (1ll << 31)) return SCFLOW_EUNSUPPORTED;
  if (!aligned16(out) || (!u8 && ((uintptr_t)frames & 3u))) return SCFLOW_EALIGN;
  PatchExtractArgs a{};
  a.frames = frames, a.frame_index = frame_index, a.geom = geom, a.valid = valid, a.out = out;
  a.F = num_frames, a.H = height, a.W = width, a.S = size, a.pad = pad;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean && c < channels ? mean[c] : 0.f;
    a.std[c] = std && c < channels ? std[c] : 1.f;
  }
  a.to_rgb = (flags & SCFLOW_PATCH_TO_RGB) != 0, a.quantize = (flags & SCFLOW_PATCH_QUANTIZE) != 0;
  a.nearest = (flags & SCFLOW_PATCH_NEAREST) != 0, a.use_lds = g_patch_lds.get() != 0;
  const dim3 grid(n * bands), block(PX_THREADS);
  const size_t lds = a.use_lds ? PX_LDS_BYTES : 0;  // the direct route keeps the CU's LDS free
  hipStream_t s = (hipStream_t)stream;
  if (u8 && channels == 3)
    hipLaunchKernelGGL((patch_extract_kernel<unsigned char, 3>), grid, block, lds, s, a);
  else if (u8)
    hipLaunchKernelGGL((patch_extract_kernel<unsigned char, 1>), grid, block, lds, s, a);
  else
    hipLaunchKernelGGL((patch_extract_kernel<float, 1>), grid, block, lds, s, a);
  return scflow_launch_status();
}
