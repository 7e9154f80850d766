// Flow validation: the GT flow with its validity filters, and the end-point-error statistics.
//
//   get_flow_from_delta_pose_and_depth            /root/reference/models/utils/pose.py:92-121
//   filter_flow_by_mask / _by_depth / _by_face_index, cal_epe
//                                                 /root/reference/models/utils/flow.py:6-88
//   eval_epe_and_occ's occlusion term             /root/reference/models/refiner/raft_refiner_flow_mask.py:256-257
//
// scflow_flow_gt is one launch, one thread per pixel: lift + reprojection with the device
// functions of lift_kernel / pose_flow_kernel (pose_dev.h; the unfiltered flow has their bits),
// then up to three filters that each decide from the pixel's unfiltered flow — 4 B read and 8 to
// 16 B written per pixel plus the filters' taps, HBM-bound, nothing staged (no reuse between
// pixels beyond what the L2 already gives the 4 bilinear taps).
//
// scflow_flow_epe is two launches: every workgroup reduces its pixels to 2 fp64 sums and 4
// integer counts (per thread in pixel order, the wave by shuffles, the 4 waves through LDS in wave
// order) and stores them; a second launch of one wave per sample adds the workgroups' partials
// in workgroup order.  No floating-point atomics: the sums have the same bits in every run.
#include "pose_dev.h"

namespace {

// ATen's grid_sample coordinates (GridSampler.h grid_sampler_unnormalize) of the reference's
// coords_grid (models/utils/warp.py:9-28): g = c·2 / max(size − 1, 1) − 1 whatever align_corners
// the sampling then uses
__device__ __forceinline__ float grid_coord(float c, int size) {
#pragma clang fp contract(off)
  return c * 2.f / (float)(size > 1 ? size - 1 : 1) - 1.f;
}
__device__ __forceinline__ float unnorm(float g, int size, bool align_corners) {
#pragma clang fp contract(off)
  return align_corners ? ((g + 1.f) / 2.f) * (float)(size - 1) : ((g + 1.f) * (float)size - 1.f) / 2.f;
}

struct MaskTap {  // gt_mask as bool / uint8 (dtype 0) or float32 (dtype 1)
  const void* p;
  int dtype;
  __device__ __forceinline__ float operator()(size_t i) const {
    return dtype ? ((const float*)p)[i] : (float)((const unsigned char*)p)[i];
  }
};
struct DepthTap {  // non-positive depths read as zero (flow.py:33-37)
  const float* p;
  __device__ __forceinline__ float operator()(size_t i) const {
    const float v = p[i];
    return v > 0.f ? v : 0.f;
  }
};
struct FaceTap {  // face indices as int32 (dtype 0) or int64 (dtype 1), compared as float32 (flow.py:50)
  const void* p;
  int dtype;
  __device__ __forceinline__ float operator()(size_t i) const {
    return dtype ? (float)((const long long*)p)[i] : (float)((const int*)p)[i];
  }
};

// grid_sample(mode='bilinear', padding_mode='zeros') of one H×W plane at (ix, iy): ATen's tap
// weights and summation order (nw, ne, sw, se), a tap outside the plane contributing nothing
template <class Tap>
__device__ __forceinline__ float sample_bilinear(const Tap& tap, size_t base, float ix, float iy,
                                                 int H, int W) {
#pragma clang fp contract(off)
  // no tap inside the plane (or a NaN coordinate): also keeps the float → int conversions in range
  if (!(ix >= -1.f && ix < (float)W && iy >= -1.f && iy < (float)H)) return 0.f;
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
  const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
  const float nw = (fx1 - ix) * (fy1 - iy), ne = (ix - fx0) * (fy1 - iy);
  const float sw = (fx1 - ix) * (iy - fy0), se = (ix - fx0) * (iy - fy0);
  const bool xa = x0 >= 0, xb = x1 < W, ya = y0 >= 0, yb = y1 < H;
  float out = 0.f;
  if (ya && xa) out += tap(base + (size_t)y0 * W + x0) * nw;
  if (ya && xb) out += tap(base + (size_t)y0 * W + x1) * ne;
  if (yb && xa) out += tap(base + (size_t)y1 * W + x0) * sw;
  if (yb && xb) out += tap(base + (size_t)y1 * W + x1) * se;
  return out;
}

// grid_sample(mode='nearest', padding_mode='zeros'): the nearest tap, ties to even (nearbyint)
template <class Tap>
__device__ __forceinline__ float sample_nearest(const Tap& tap, size_t base, float ix, float iy,
                                                int H, int W) {
  const float rx = nearbyintf(ix), ry = nearbyintf(iy);
  if (!(rx >= 0.f && rx <= (float)(W - 1) && ry >= 0.f && ry <= (float)(H - 1))) return 0.f;
  return tap(base + (size_t)(int)ry * W + (int)rx);
}

__global__ __launch_bounds__(256) void flow_gt_kernel(const scflow_flow_gt_args a) {
  __shared__ float sl[21];  // Kinv[9] Rinv[9] t_ref[3]
  __shared__ float sp[21];  // R_gt[9] t_gt[3] K[9]
  const int n = blockIdx.y;
  const int H = a.h, W = a.w, HW = H * W;
  if (!a.flow_in) {
    if (threadIdx.x == 0) lift_prologue(sl, n, a.K, a.R_ref, a.t_ref);
    pose_prologue(sp, n, nullptr, nullptr, a.R_gt, a.t_gt, a.K, nullptr, nullptr, 10.f, 0, 0, false);
  }
  const size_t plane = (size_t)n * HW;
  const float inv = a.invalid_num;
  const MaskTap mask{a.gt_mask, a.mask_dtype};
  const DepthTap depth1{a.depth1};
  const FaceTap face2{a.face_index2, a.face_dtype};
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
#pragma clang fp contract(off)
    const int X = p % W, Y = p / W;
    float fx, fy;
    if (a.flow_in) {
      fx = a.flow_in[plane * 2 + p];
      fy = a.flow_in[plane * 2 + HW + p];
    } else {
      proj_flow(sp, lift_point(sl, a.depth[plane + p], X, Y), X, Y, inv, fx, fy);
    }
    if (a.flow) {
      a.flow[plane * 2 + p] = fx;
      a.flow[plane * 2 + HW + p] = fy;
    }
    if (!a.flow_filtered) continue;
    const bool bad0 = fx >= inv && fy >= inv;  // already invalid: what every reference filter starts from
    const float gx = grid_coord((float)X + fx, W), gy = grid_coord((float)Y + fy, H);
    bool bad = false;
    if (a.gt_mask) {  // align_corners=False on a grid normalised for align_corners=True: the reference's
      const float m = sample_bilinear(mask, plane, unnorm(gx, W, false), unnorm(gy, H, false), H, W);
      bad = bad || bad0 || m < 0.9f;
    }
    if (a.depth1) {
      const float wd = sample_bilinear(depth1, plane, unnorm(gx, W, true), unnorm(gy, H, true), H, W);
      float d0 = a.depth[plane + p];
      d0 = d0 > 0.f ? d0 : 0.f;
      const bool consistent = fabsf(d0 - wd) / (d0 + 0.1f) < a.depth_thr;
      bad = bad || (a.depth_combine == SCFLOW_FLOW_DEPTH_OR ? (bad0 || !consistent)
                                                           : (bad0 && !consistent));
    }
    if (a.face_index1) {
      const float s = sample_nearest(face2, plane, unnorm(gx, W, true), unnorm(gy, H, true), H, W);
      const FaceTap face1{a.face_index1, a.face_dtype};
      bad = bad || bad0 || !(s == face1(plane + p));
    }
    a.flow_filtered[plane * 2 + p] = bad ? inv : fx;
    a.flow_filtered[plane * 2 + HW + p] = bad ? inv : fy;
  }
}

// ------------------------------------------------------------------------------------------ EPE
constexpr int EPE_MAX_BLOCKS = 64;  // workgroups per sample (their partials: one wave's second pass)

__host__ __device__ inline int epe_blocks(long long hw) {
  const long long b = (hw + 255) / 256;
  return (int)(b < EPE_MAX_BLOCKS ? b : EPE_MAX_BLOCKS);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// partials of sample n, workgroup b: psum[(n·nb + b)·2 + {0: error, 1: occlusion}],
// pcnt[(n·nb + b)·4 + {0: valid, 1..3: below threshold k}]
__global__ __launch_bounds__(256) void flow_epe_kernel(const scflow_flow_epe_args a, double* psum,
                                                       int* pcnt) {
  __shared__ double ssum[4][2];
  __shared__ int scnt[4][4];
  const int n = blockIdx.y;
  const int HW = a.h * a.w;
  const size_t plane = (size_t)n * HW;
  double se = 0.0, so = 0.0;
  int c[4] = {0, 0, 0, 0};
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
#pragma clang fp contract(off)
    const float tx = a.flow_tgt[plane * 2 + p], ty = a.flow_tgt[plane * 2 + HW + p];
    const float dx = tx - a.flow_pred[plane * 2 + p], dy = ty - a.flow_pred[plane * 2 + HW + p];
    const bool inside = sqrtf(tx * tx + ty * ty) < a.max_flow;
    const bool valid = inside && (!a.mask || a.mask[plane + p] >= 0.5f);
    const float err = sqrtf(dx * dx + dy * dy);
    if (a.err_map) a.err_map[plane + p] = valid ? err : err * 0.f;  // err · 0: the reference's NaN stays
    if (valid) {
      se += (double)err;
      c[0] += 1;
      for (int k = 0; k < 3; ++k) c[k + 1] += err < a.thresh[k] ? 1 : 0;
    }
    if (a.occ_pred) so += (double)fabsf((inside ? 1.f : 0.f) - a.occ_pred[plane + p]);
  }
  if (!psum) return;  // the error map alone
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  se = wave_sum(se);
  so = wave_sum(so);
  for (int k = 0; k < 4; ++k) c[k] = wave_sum(c[k]);
  if (lane == 0) {
    ssum[wave][0] = se;
    ssum[wave][1] = so;
    for (int k = 0; k < 4; ++k) scnt[wave][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const size_t b = (size_t)n * gridDim.x + blockIdx.x;
    const int k = threadIdx.x;
    if (k < 2)
      psum[b * 2 + k] = ((ssum[0][k] + ssum[1][k]) + ssum[2][k]) + ssum[3][k];
    else
      pcnt[b * 4 + (k - 2)] = scnt[0][k - 2] + scnt[1][k - 2] + scnt[2][k - 2] + scnt[3][k - 2];
  }
}

__global__ __launch_bounds__(64) void flow_epe_final_kernel(const double* __restrict__ psum,
                                                            const int* __restrict__ pcnt, int nb,
                                                            double* __restrict__ sums,
                                                            int* __restrict__ counts) {
  const int n = blockIdx.x, k = threadIdx.x;
  if (k < 2) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += psum[((size_t)n * nb + b) * 2 + k];
    sums[n * 2 + k] = s;
  } else if (k < 6) {
    int s = 0;
    for (int b = 0; b < nb; ++b) s += pcnt[((size_t)n * nb + b) * 4 + (k - 2)];
    counts[n * 4 + (k - 2)] = s;
  }
}

inline bool shape_ok(int n, int h, int w) { return n > 0 && h > 0 && w > 0; }

}  // namespace

SCFLOW_API int scflow_flow_gt(const scflow_flow_gt_args* args, void* stream) {
  if (!args) return SCFLOW_EINVAL;
  const scflow_flow_gt_args& a = *args;
  if (!shape_ok(a.n, a.h, a.w)) return SCFLOW_EINVAL;
  const bool poses = a.K || a.R_ref || a.t_ref || a.R_gt || a.t_gt;
  if (a.flow_in ? poses : !(a.depth && a.K && a.R_ref && a.t_ref && a.R_gt && a.t_gt))
    return SCFLOW_EINVAL;  // one flow source: the poses (with the depth) or flow_in
  if (!a.flow && !a.flow_filtered) return SCFLOW_EINVAL;
  if (a.depth1 && !a.depth) return SCFLOW_EINVAL;
  if (!a.face_index1 != !a.face_index2) return SCFLOW_EINVAL;
  if ((a.mask_dtype | a.face_dtype) & ~1) return SCFLOW_EINVAL;
  if (a.depth_combine != SCFLOW_FLOW_DEPTH_OR && a.depth_combine != SCFLOW_FLOW_DEPTH_REFERENCE)
    return SCFLOW_EINVAL;
  if (a.flow_in && (a.flow_in == a.flow || a.flow_in == a.flow_filtered)) return SCFLOW_EINVAL;
  if (a.flow && a.flow == a.flow_filtered) return SCFLOW_EINVAL;
  const long long hw = (long long)a.h * a.w;
  if (hw >= (1ll << 30) || a.n > 65535) return SCFLOW_EUNSUPPORTED;
  const int bx = ceil_div(hw, 256) < 256 ? ceil_div(hw, 256) : 256;
  flow_gt_kernel<<<dim3(bx, a.n), 256, 0, (hipStream_t)stream>>>(a);
  return scflow_launch_status();
}

SCFLOW_API long long scflow_flow_epe_workspace(int n, int h, int w) {
  if (!shape_ok(n, h, w)) return SCFLOW_EINVAL;
  return (long long)n * epe_blocks((long long)h * w) * (2 * sizeof(double) + 4 * sizeof(int));
}

SCFLOW_API int scflow_flow_epe(const scflow_flow_epe_args* args, void* stream) {
  if (!args) return SCFLOW_EINVAL;
  const scflow_flow_epe_args& a = *args;
  if (!shape_ok(a.n, a.h, a.w) || !a.flow_tgt || !a.flow_pred) return SCFLOW_EINVAL;
  if (!a.sums != !a.counts || (!a.sums && !a.err_map)) return SCFLOW_EINVAL;
  const long long hw = (long long)a.h * a.w;
  if (hw >= (1ll << 30) || a.n > 65535) return SCFLOW_EUNSUPPORTED;
  const int nb = epe_blocks(hw);
  double* psum = nullptr;
  int* pcnt = nullptr;
  if (a.sums) {
    if (!a.workspace || ((uintptr_t)a.workspace & 7u)) return a.workspace ? SCFLOW_EALIGN : SCFLOW_EINVAL;
    if (a.workspace_bytes < scflow_flow_epe_workspace(a.n, a.h, a.w)) return SCFLOW_EINVAL;
    psum = (double*)a.workspace;
    pcnt = (int*)(psum + (size_t)a.n * nb * 2);
  }
  flow_epe_kernel<<<dim3(nb, a.n), 256, 0, (hipStream_t)stream>>>(a, psum, pcnt);
  int st = scflow_launch_status();
  if (st != SCFLOW_OK || !a.sums) return st;
  flow_epe_final_kernel<<<a.n, 64, 0, (hipStream_t)stream>>>(psum, pcnt, nb, a.sums, a.counts);
  return scflow_launch_status();
}
