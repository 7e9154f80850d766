// BOP pose errors (bop_toolkit's pose_error.py, BOP19 settings; DESIGN.md §22 has the contract):
//
//   scflow_pose_err_sym  MSSD and MSPD of N (estimate, ground truth) pairs in one pass:
//                        min over the class's symmetry transforms of max over its vertices.
//                        No [N, S, P] intermediate exists: a workgroup owns one estimate and a
//                        slice of its symmetries, takes them four at a time (their R̄·S | R̄·S_t + t̄
//                        built once in LDS and held in scalar registers), strides the vertices
//                        with its lanes, reduces the maxima per wave by shuffles and across waves
//                        through LDS, and combines the minimum over symmetries across workgroups
//                        with an integer atomicMin on the float's bits (errors are ≥ 0, so the
//                        unsigned order is the float order).
//   scflow_vsd_counts    the VSD pixel counts (|U|, |I|, cost_k) of N pairs in one launch:
//                        per-lane integer counters, a shuffle reduction per wave, LDS across
//                        waves, one integer atomic per workgroup and counter.
//
// Max, min and integer sums do not depend on order: both results are bitwise reproducible.  Every
// product-sum is an explicit fmaf with contraction off, so MSSD (MSPD) has the same bits whether
// or not the other one is computed in the same launch.
#include "common.h"

#include <limits.h>

namespace {

constexpr int kSymChunk = 4;    // symmetries a workgroup holds in registers at a time
constexpr int kMaxSlices = 64;  // workgroups that share one estimate's symmetries, at most
constexpr int kMaxTaus = 16;

__device__ __forceinline__ float uniformf(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// r = A·x + b with A row-major 3×3 at a[0..8] and b given apart
__device__ __forceinline__ void affine3(const float* a, float b0, float b1, float b2, float x,
                                        float y, float z, float& r0, float& r1, float& r2) {
  r0 = fmaf(a[2], z, fmaf(a[1], y, fmaf(a[0], x, b0)));
  r1 = fmaf(a[5], z, fmaf(a[4], y, fmaf(a[3], x, b1)));
  r2 = fmaf(a[8], z, fmaf(a[7], y, fmaf(a[6], x, b2)));
}

__global__ void fill_inf_kernel(float* a, float* b, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (a) a[i] = __int_as_float(0x7f800000);
  if (b) b[i] = __int_as_float(0x7f800000);
}

// grid (n, slices): workgroup (i, y) takes symmetries [y·per, (y+1)·per) of estimate i's class.
// A label outside [0, C), a class without vertices or without symmetries: the outputs keep their
// +inf.  Vertices at and past counts[label] are never read.
template <bool DO_S, bool DO_P>
__global__ __launch_bounds__(256) void pose_err_sym_kernel(
    const float* __restrict__ points, const int* __restrict__ counts, int C, int max_points,
    const float* __restrict__ sym, const int* __restrict__ sym_offset, int total_syms,
    const int* __restrict__ labels, const float* __restrict__ R_est,
    const float* __restrict__ t_est, const float* __restrict__ R_gt,
    const float* __restrict__ t_gt, const float* __restrict__ Kmat, unsigned* __restrict__ mssd,
    unsigned* __restrict__ mspd) {
#pragma clang fp contract(off)
  __shared__ float sm[kSymChunk][12];
  __shared__ float red[4][2 * kSymChunk];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int lab = labels[n];
  if (lab < 0 || lab >= C) return;
  int cnt = counts[lab];
  cnt = cnt < max_points ? cnt : max_points;
  if (cnt <= 0) return;
  int o0 = sym_offset[lab], o1 = sym_offset[lab + 1];
  o0 = o0 < 0 ? 0 : o0;
  o1 = o1 > total_syms ? total_syms : o1;
  const int S = o1 - o0;
  if (S <= 0) return;
  const int per = (S + gridDim.y - 1) / gridDim.y;
  const int s0 = blockIdx.y * per;
  const int s1 = s0 + per < S ? s0 + per : S;
  if (s0 >= s1) return;

  float Re[9], te[3], Rg[9], tg[3], K[9];
  for (int e = 0; e < 9; ++e) {
    Re[e] = R_est[(size_t)n * 9 + e];
    Rg[e] = R_gt[(size_t)n * 9 + e];
    K[e] = DO_P ? Kmat[(size_t)n * 9 + e] : 0.f;
  }
  for (int e = 0; e < 3; ++e) {
    te[e] = t_est[(size_t)n * 3 + e];
    tg[e] = t_gt[(size_t)n * 3 + e];
  }
  const float* __restrict__ pts = points + (size_t)lab * max_points * 3;
  const float inf = __int_as_float(0x7f800000);
  float best_s = inf, best_p = inf;  // thread 0's: the minimum over this workgroup's symmetries

  for (int c0 = s0; c0 < s1; c0 += kSymChunk) {
    __syncthreads();  // the previous chunk's sm and red have been read
    if (tid < kSymChunk * 12) {
      // [R̄·S_R | R̄·S_t + t̄] of symmetry c0 + j; past the slice's end, its last one once more
      // (a duplicate does not move a minimum)
      const int j = tid / 12, e = tid - j * 12, r = e >> 2, col = e & 3;
      const int s = c0 + j < s1 ? c0 + j : s1 - 1;
      const float* __restrict__ T = sym + (size_t)(o0 + s) * 12;
      float v = fmaf(Rg[r * 3 + 2], T[8 + col], fmaf(Rg[r * 3 + 1], T[4 + col], Rg[r * 3] * T[col]));
      if (col == 3) v += tg[r];
      sm[j][e] = v;
    }
    __syncthreads();
    float A[kSymChunk][9], b[kSymChunk][3];
    for (int j = 0; j < kSymChunk; ++j)
      for (int r = 0; r < 3; ++r) {
        for (int col = 0; col < 3; ++col) A[j][r * 3 + col] = uniformf(sm[j][r * 4 + col]);
        b[j][r] = uniformf(sm[j][r * 4 + 3]);
      }
    float ms[kSymChunk], mp[kSymChunk];
    for (int j = 0; j < kSymChunk; ++j) ms[j] = mp[j] = 0.f;

    for (int i = tid; i < cnt; i += 256) {
      const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
      float px, py, pz, ue = 0.f, ve = 0.f;
      affine3(Re, te[0], te[1], te[2], x, y, z, px, py, pz);
      if (DO_P) {
        float hx, hy, hz;
        affine3(K, 0.f, 0.f, 0.f, px, py, pz, hx, hy, hz);
        const float ih = __builtin_amdgcn_rcpf(hz);
        ue = hx * ih;
        ve = hy * ih;
      }
#pragma unroll
      for (int j = 0; j < kSymChunk; ++j) {
        float qx, qy, qz;
        affine3(A[j], b[j][0], b[j][1], b[j][2], x, y, z, qx, qy, qz);
        if (DO_S) {
          const float dx = px - qx, dy = py - qy, dz = pz - qz;
          ms[j] = fmaxf(ms[j], fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        }
        if (DO_P) {
          float gx, gy, gz;
          affine3(K, 0.f, 0.f, 0.f, qx, qy, qz, gx, gy, gz);
          const float ig = __builtin_amdgcn_rcpf(gz);
          const float du = ue - gx * ig, dv = ve - gy * ig;
          mp[j] = fmaxf(mp[j], fmaf(dv, dv, du * du));
        }
      }
    }

    const int lane = tid & 63, wave = tid >> 6;
    for (int j = 0; j < kSymChunk; ++j) {
      const float a = DO_S ? wave_max(ms[j]) : 0.f;
      const float c = DO_P ? wave_max(mp[j]) : 0.f;
      if (lane == 0) {
        red[wave][j] = a;
        red[wave][kSymChunk + j] = c;
      }
    }
    __syncthreads();
    if (tid == 0)
      for (int j = 0; j < kSymChunk; ++j) {
        // the square root is monotonic: the maximum of the squares is the square of the maximum
        const float a = fmaxf(fmaxf(red[0][j], red[1][j]), fmaxf(red[2][j], red[3][j]));
        const float c = fmaxf(fmaxf(red[0][kSymChunk + j], red[1][kSymChunk + j]),
                              fmaxf(red[2][kSymChunk + j], red[3][kSymChunk + j]));
        best_s = fminf(best_s, sqrtf(a));
        best_p = fminf(best_p, sqrtf(c));
      }
  }
  if (tid == 0) {
    if (DO_S) atomicMin(mssd + n, __float_as_uint(best_s));
    if (DO_P) atomicMin(mspd + n, __float_as_uint(best_p));
  }
}

// grid (pixel blocks, n); V = pixels per load (4: float4 loads, h·w a multiple of 4 and the three
// maps 16-byte aligned).  A frame_index outside [0, F) leaves the pair's counts 0.
template <int V>
__global__ __launch_bounds__(256) void vsd_counts_kernel(
    const float* __restrict__ depth_est, const float* __restrict__ depth_gt,
    const float* __restrict__ depth_test, const int* __restrict__ frame_index, int F,
    const float* __restrict__ Kmat, const float* __restrict__ diameter,
    const float* __restrict__ taus, int n_taus, float delta, int h, int w,
    int* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ int red[4][2 + kMaxTaus];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int f = frame_index[n];
  if (f < 0 || f >= F) return;
  const int hw = h * w;
  const float* __restrict__ de = depth_est + (size_t)n * hw;
  const float* __restrict__ dg = depth_gt + (size_t)n * hw;
  const float* __restrict__ dt = depth_test + (size_t)f * hw;
  const float fx = Kmat[(size_t)n * 9], cx = Kmat[(size_t)n * 9 + 2];
  const float fy = Kmat[(size_t)n * 9 + 4], cy = Kmat[(size_t)n * 9 + 5];
  const float ifx = 1.f / fx, ify = 1.f / fy;
  const float diam = diameter ? diameter[n] : 1.f;
  float tau[kMaxTaus];
  for (int k = 0; k < kMaxTaus; ++k) tau[k] = k < n_taus ? taus[k] : 0.f;
  int c[2 + kMaxTaus];
  for (int k = 0; k < 2 + kMaxTaus; ++k) c[k] = 0;

  for (int p0 = (blockIdx.x * 256 + tid) * V; p0 < hw; p0 += gridDim.x * 256 * V) {
    float E[V], G[V], T[V];
    if (V == 4) {
      const floatx4 e4 = *(const floatx4*)(de + p0), g4 = *(const floatx4*)(dg + p0),
                    t4 = *(const floatx4*)(dt + p0);
      for (int e = 0; e < V; ++e) E[e] = e4[e], G[e] = g4[e], T[e] = t4[e];
    } else {
      for (int e = 0; e < V; ++e) E[e] = de[p0 + e], G[e] = dg[p0 + e], T[e] = dt[p0 + e];
    }
    int y = p0 / w, x = p0 - y * w;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      // a pixel that neither render covers is visible in neither mask and enters no count: most
      // of a frame, and whole waves of it, stop here
      if (E[e] > 0.f || G[e] > 0.f) {
        // depth → distance from the camera centre: the same factor for the three maps of a pixel
        const float ax = ((float)x - cx) * ifx, ay = ((float)y - cy) * ify;
        const float s = sqrtf(fmaf(ax, ax, fmaf(ay, ay, 1.f)));
        const float me = E[e] * s, mg = G[e] * s, mt = T[e] * s;
        const bool unseen = mt == 0.f;
        const bool vg = (mg - mt <= delta || unseen) && mg > 0.f;
        const bool ve = ((me - mt <= delta || unseen) && me > 0.f) || (vg && me > 0.f);
        const bool in = vg && ve;
        c[0] += (vg || ve) ? 1 : 0;
        c[1] += in ? 1 : 0;
        const float a = fabsf(mg - me);
        const float r = diameter ? a / diam : a;
#pragma unroll
        for (int k = 0; k < kMaxTaus; ++k) c[2 + k] += (in && k < n_taus && r >= tau[k]) ? 1 : 0;
      }
      if (++x == w) {
        x = 0;
        ++y;
      }
    }
  }

  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 2 + kMaxTaus; ++k) {
    const int v = wave_sum(c[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (tid < 2 + n_taus) {
    const int v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    if (v) atomicAdd(counts + (size_t)n * (2 + n_taus) + tid, v);
  }
}

}  // namespace

SCFLOW_API int scflow_pose_err_sym(const float* points, const int* counts, int num_classes,
                                   int max_points, const float* sym, const int* sym_offset,
                                   int total_syms, const int* labels, const float* R_est,
                                   const float* t_est, const float* R_gt, const float* t_gt,
                                   const float* K, float* mssd, float* mspd, int n, void* stream) {
  if (!points || !counts || !sym || !sym_offset || !labels || !R_est || !t_est || !R_gt || !t_gt ||
      (!mssd && !mspd) || (mspd && !K) || num_classes < 1 || max_points < 1 || total_syms < 1 ||
      n < 0)
    return SCFLOW_EINVAL;
  if (n == 0) return SCFLOW_OK;
  if (max_points > INT_MAX / 3) return SCFLOW_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  fill_inf_kernel<<<ceil_div(n, 256), 256, 0, st>>>(mssd, mspd, n);
  // enough workgroups to fill the chip at small n, never more slices than chunks of symmetries
  int slices = ceil_div(4 * device_cus(), n);
  const int chunks = ceil_div(total_syms, kSymChunk);
  slices = slices < chunks ? slices : chunks;
  slices = slices < kMaxSlices ? slices : kMaxSlices;
  const dim3 grid(n, slices);
  unsigned* us = (unsigned*)mssd;
  unsigned* up = (unsigned*)mspd;
#define SCFLOW_POSE_ERR_LAUNCH(S_, P_)                                                          \
  pose_err_sym_kernel<S_, P_><<<grid, 256, 0, st>>>(points, counts, num_classes, max_points, sym, \
                                                    sym_offset, total_syms, labels, R_est, t_est, \
                                                    R_gt, t_gt, K, us, up)
  if (mssd && mspd)
    SCFLOW_POSE_ERR_LAUNCH(true, true);
  else if (mssd)
    SCFLOW_POSE_ERR_LAUNCH(true, false);
  else
    SCFLOW_POSE_ERR_LAUNCH(false, true);
#undef SCFLOW_POSE_ERR_LAUNCH
  return scflow_launch_status();
}

SCFLOW_API int scflow_vsd_counts(const float* depth_est, const float* depth_gt,
                                 const float* depth_test, const int* frame_index, const float* K,
                                 const float* diameter, const float* taus, int n_taus, float delta,
                                 int* counts, int n, int n_frames, int h, int w, void* stream) {
  if (!depth_est || !depth_gt || !depth_test || !frame_index || !K || !taus || !counts || n < 0 ||
      n_frames < 1 || h < 1 || w < 1 || n_taus < 1 || n_taus > kMaxTaus)
    return SCFLOW_EINVAL;
  if (n == 0) return SCFLOW_OK;
  if ((long long)h * w > (1LL << 30) || n > 65535) return SCFLOW_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * (2 + n_taus) * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const int hw = h * w;
  const bool vec = hw % 4 == 0 && aligned16(depth_est) && aligned16(depth_gt) && aligned16(depth_test);
  // eight pixels per lane and pass, unless that leaves the chip short of workgroups
  const int per_block = 256 * 8;
  int gx = ceil_div(hw, per_block);
  const int want = ceil_div(8 * device_cus(), n);
  const int most = ceil_div(hw, 256 * (vec ? 4 : 1));
  if (gx < want) gx = want < most ? want : most;
  const dim3 grid(gx, n);
  if (vec)
    vsd_counts_kernel<4><<<grid, 256, 0, st>>>(depth_est, depth_gt, depth_test, frame_index,
                                               n_frames, K, diameter, taus, n_taus, delta, h, w,
                                               counts);
  else
    vsd_counts_kernel<1><<<grid, 256, 0, st>>>(depth_est, depth_gt, depth_test, frame_index,
                                               n_frames, K, diameter, taus, n_taus, delta, h, w,
                                               counts);
  return scflow_launch_status();
}
