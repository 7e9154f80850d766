// a8–a11: pose update, 2D-3D lift, pose-induced flow, flow resampling, layout transposes.
//
//   get_pose_from_delta_pose (ortho6d, exp)     /root/reference/models/utils/pose.py:124-169
//   cal_3d_2d_corr / lift_2d_to_3d              /root/reference/models/utils/pose.py:26-64
//   get_flow_from_delta_pose_and_points         /root/reference/models/utils/pose.py:66-88
//   flow ↓8 / flow, mask ↑8 (F.interpolate bilinear, align_corners=True)
//                                               /root/reference/models/decoder/scflow_decoder.py:197-198, 223-228
//
// The reference enumerates foreground pixels with torch.nonzero (a host sync per sample) and
// scatters the reprojected flow back with index_put inside a Python loop over the batch.  Here
// the lift is dense and predicated (one float4 {X,Y,Z,valid} per pixel, once per forward), and
// every refinement iteration is ONE launch that recomputes the pose update in its prologue
// (a few hundred flops per workgroup, kept in LDS) and reprojects every pixel: HBM-bound,
// 16 B read + 8 B written per pixel.
#include "pose_dev.h"

namespace {

__global__ void pose_update_kernel(const float* drot6, const float* dt, const float* Rs,
                                   const float* ts, float* Rd, float* td, int n, float weight,
                                   int depth_transform) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pose_update_one(drot6 + pose_rot_dim(depth_transform) * i, dt + 3 * i, Rs + 9 * i, ts + 3 * i,
                  Rd + 9 * i, td + 3 * i, weight, depth_transform);
}

__global__ __launch_bounds__(256) void lift_kernel(const float* __restrict__ depth,
                                                   const float* __restrict__ K,
                                                   const float* __restrict__ R,
                                                   const float* __restrict__ t,
                                                   floatx4* __restrict__ pts, int H, int W) {
  __shared__ float sh[21];  // Kinv[9], Rinv[9], t[3]
  const int n = blockIdx.y;
  if (threadIdx.x == 0) lift_prologue(sh, n, K, R, t);
  __syncthreads();
  const int HW = H * W;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256)
    pts[(size_t)n * HW + p] = lift_point(sh, depth[(size_t)n * HW + p], p % W, p / W);
}

// flow[n][0/1][p] from pose (R,t) in LDS; `upd` != 0: compute (R,t) from the delta first
__global__ __launch_bounds__(256) void pose_flow_kernel(
    const float* __restrict__ drot6, const float* __restrict__ dtv, const float* __restrict__ Rsrc,
    const float* __restrict__ tsrc, const float* __restrict__ K, const floatx4* __restrict__ pts,
    float* __restrict__ Rout, float* __restrict__ tout, float* __restrict__ flow, int H, int W,
    float weight, int depth_transform, float invalid, int upd) {
  __shared__ float sh[21];  // R[9] t[3] K[9]
  const int n = blockIdx.y;
  pose_prologue(sh, n, drot6, dtv, Rsrc, tsrc, K, Rout, tout, weight, depth_transform, upd,
                blockIdx.x == 0);
  const int HW = H * W;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    float fx, fy;
    proj_flow(sh, pts[(size_t)n * HW + p], p % W, p / W, invalid, fx, fy);
    flow[((size_t)n * 2 + 0) * HW + p] = fx;
    flow[((size_t)n * 2 + 1) * HW + p] = fy;
  }
}

__global__ __launch_bounds__(256) void downsample_kernel(const float* __restrict__ flow,
                                                         float* __restrict__ o0, int s0,
                                                         float* __restrict__ o1, int s1,
                                                         const float* __restrict__ mask,
                                                         float* __restrict__ om, int sm, int N,
                                                         int H, int W, int h, int w, float vs) {
#pragma clang fp contract(off)
  const long long total = (long long)N * h * w;
  const long long idx = blockIdx.x * 256LL + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % w);
  const long long t = idx / w;
  const int y = (int)(t % h);
  const int n = (int)(t / h);
  const Lin ly = lin_src(y, H, h), lx = lin_src(x, W, w);
  float r[2];
  for (int c = 0; c < 2; ++c) {
    const float* f = flow + ((size_t)n * 2 + c) * H * W;
    const float v = bilerp(f[(size_t)ly.i0 * W + lx.i0], f[(size_t)ly.i0 * W + lx.i1],
                           f[(size_t)ly.i1 * W + lx.i0], f[(size_t)ly.i1 * W + lx.i1], ly, lx);
    r[c] = vs * v;
  }
  o0[idx * s0 + 0] = r[0];
  o0[idx * s0 + 1] = r[1];
  // masked (scflow_flow_downsample_masked): o0 unmasked, o1 and om times the pixel's mask
  const float mk = mask ? mask[idx] : 1.f;
  if (o1) {
    o1[idx * s1 + 0] = r[0] * mk;
    o1[idx * s1 + 1] = r[1] * mk;
  }
  if (om) {
    om[idx * sm + 0] = r[0] * mk;
    om[idx * sm + 1] = r[1] * mk;
  }
}

__global__ __launch_bounds__(256) void upsample_kernel(const float* __restrict__ lr,
                                                       const float* __restrict__ delta,
                                                       const float* __restrict__ mask,
                                                       float* __restrict__ fo,
                                                       float* __restrict__ mo, int N, int h, int w,
                                                       int H, int W, float vs) {
#pragma clang fp contract(off)
  const long long total = (long long)N * H * W;
  const long long idx = blockIdx.x * 256LL + threadIdx.x;
  if (idx >= total) return;
  const int X = (int)(idx % W);
  const long long t = idx / W;
  const int Y = (int)(t % H);
  const int n = (int)(t / H);
  const Lin ly = lin_src(Y, h, H), lx = lin_src(X, w, W);
  const size_t b = (size_t)n * h * w;
  const size_t i00 = b + (size_t)ly.i0 * w + lx.i0, i01 = b + (size_t)ly.i0 * w + lx.i1;
  const size_t i10 = b + (size_t)ly.i1 * w + lx.i0, i11 = b + (size_t)ly.i1 * w + lx.i1;
  for (int c = 0; c < 2; ++c) {
    float v00 = lr[i00 * 2 + c], v01 = lr[i01 * 2 + c], v10 = lr[i10 * 2 + c], v11 = lr[i11 * 2 + c];
    if (delta) {
      v00 = v00 + delta[i00 * 2 + c];
      v01 = v01 + delta[i01 * 2 + c];
      v10 = v10 + delta[i10 * 2 + c];
      v11 = v11 + delta[i11 * 2 + c];
    }
    fo[((size_t)n * 2 + c) * H * W + (size_t)Y * W + X] = vs * bilerp(v00, v01, v10, v11, ly, lx);
  }
  if (mask && mo)
    mo[(size_t)n * H * W + (size_t)Y * W + X] = bilerp(mask[i00], mask[i01], mask[i10], mask[i11], ly, lx);
}

__global__ __launch_bounds__(256) void pose_step_kernel(PoseStepArgs a) {
  __shared__ float sh[21];
  __shared__ float hs[16 + 16 * 4 + 21];  // fused heads: results, the 4 waves' partial sums,
                                          // then the prefetched R, t, K
  pose_step_body(a, sh, blockIdx.x, blockIdx.y, threadIdx.x, 256, false, hs);
}

// batched 2-D transpose through a padded LDS tile
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in,
                                                        float* __restrict__ out, int A, int B,
                                                        long long ins, int ias, long long ons,
                                                        int obs) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int a0 = blockIdx.y * 32, b0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 × 8
  for (int k = ty; k < 32; k += 8) {
    const int a = a0 + k, b = b0 + tx;
    if (a < A && b < B) tile[k][tx] = in[n * ins + (long long)a * ias + b];
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int b = b0 + k, a = a0 + tx;
    if (a < A && b < B) out[n * ons + (long long)b * obs + a] = tile[tx][k];
  }
}

}  // namespace

SCFLOW_API int scflow_pose_update(const float* drot6, const float* dt, const float* R_src,
                                  const float* t_src, float* R_dst, float* t_dst, int n,
                                  float weight, int depth_transform, void* stream) {
  if (!drot6 || !dt || !R_src || !t_src || !R_dst || !t_dst || n <= 0 ||
      !pose_mode_ok(depth_transform))
    return SCFLOW_EINVAL;
  pose_update_kernel<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(drot6, dt, R_src, t_src, R_dst,
                                                                   t_dst, n, weight, depth_transform);
  return scflow_launch_status();
}

SCFLOW_API int scflow_lift_points(const float* depth, const float* K, const float* R,
                                  const float* t, float* points, int n, int h, int w,
                                  void* stream) {
  if (!depth || !K || !R || !t || !points || n <= 0 || h <= 0 || w <= 0) return SCFLOW_EINVAL;
  if (!aligned16(points)) return SCFLOW_EALIGN;
  const int bx = ceil_div((long long)h * w, 256) < 256 ? ceil_div((long long)h * w, 256) : 256;
  lift_kernel<<<dim3(bx, n), 256, 0, (hipStream_t)stream>>>(depth, K, R, t, (floatx4*)points, h, w);
  return scflow_launch_status();
}

SCFLOW_API int scflow_pose_flow(const float* R, const float* t, const float* K,
                                const float* points, float* flow, int n, int h, int w,
                                float invalid_num, void* stream) {
  if (!R || !t || !K || !points || !flow || n <= 0 || h <= 0 || w <= 0) return SCFLOW_EINVAL;
  if (!aligned16(points)) return SCFLOW_EALIGN;
  const int bx = ceil_div((long long)h * w, 256) < 256 ? ceil_div((long long)h * w, 256) : 256;
  pose_flow_kernel<<<dim3(bx, n), 256, 0, (hipStream_t)stream>>>(
      nullptr, nullptr, R, t, K, (const floatx4*)points, nullptr, nullptr, flow, h, w, 10.f, 0,
      invalid_num, 0);
  return scflow_launch_status();
}

SCFLOW_API int scflow_pose_update_flow(const float* drot6, const float* dt, const float* R_src,
                                       const float* t_src, const float* K, const float* points,
                                       float* R_dst, float* t_dst, float* flow, int n, int h,
                                       int w, float weight, int depth_transform,
                                       float invalid_num, void* stream) {
  if (!drot6 || !dt || !R_src || !t_src || !K || !points || !R_dst || !t_dst || !flow || n <= 0 ||
      h <= 0 || w <= 0 || !pose_mode_ok(depth_transform))
    return SCFLOW_EINVAL;
  if (!aligned16(points)) return SCFLOW_EALIGN;
  const int bx = ceil_div((long long)h * w, 256) < 256 ? ceil_div((long long)h * w, 256) : 256;
  pose_flow_kernel<<<dim3(bx, n), 256, 0, (hipStream_t)stream>>>(
      drot6, dt, R_src, t_src, K, (const floatx4*)points, R_dst, t_dst, flow, h, w, weight,
      depth_transform, invalid_num, 1);
  return scflow_launch_status();
}

SCFLOW_API int scflow_flow_downsample(const float* flow, float* out0, int s0, float* out1, int s1,
                                      int n, int H, int W, int h, int w, float value_scale,
                                      void* stream) {
  if (!flow || !out0 || s0 < 2 || (out1 && s1 < 2) || n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0)
    return SCFLOW_EINVAL;
  const long long total = (long long)n * h * w;
  downsample_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      flow, out0, s0, out1, s1, nullptr, nullptr, 0, n, H, W, h, w, value_scale);
  return scflow_launch_status();
}

// the unfused tail's ↓8 flow under mask_flow: out0 ← the unmasked flow (the lookup's), out1 and
// outm ← flow · mask (mask: [n·h·w]); mask NULL: scflow_flow_downsample (+ a copy in outm)
SCFLOW_API int scflow_flow_downsample_masked(const float* flow, float* out0, int s0, float* out1,
                                             int s1, const float* mask, float* outm, int sm, int n,
                                             int H, int W, int h, int w, float value_scale,
                                             void* stream) {
  if (!flow || !out0 || s0 < 2 || (out1 && s1 < 2) || (outm && sm < 2) || n <= 0 || H <= 0 ||
      W <= 0 || h <= 0 || w <= 0)
    return SCFLOW_EINVAL;
  const long long total = (long long)n * h * w;
  downsample_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      flow, out0, s0, out1, s1, mask, outm, sm, n, H, W, h, w, value_scale);
  return scflow_launch_status();
}

SCFLOW_API int scflow_flow_upsample(const float* lr, const float* delta, const float* mask,
                                    float* flow_out, float* mask_out, int n, int h, int w, int H,
                                    int W, float value_scale, void* stream) {
  if (!lr || !flow_out || n <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return SCFLOW_EINVAL;
  const long long total = (long long)n * H * W;
  upsample_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      lr, delta, mask, flow_out, mask_out, n, h, w, H, W, value_scale);
  return scflow_launch_status();
}

// The pose step's one launcher: the four positional entries below and scflow_pose_step_call fill
// the public struct and end here.  Accepts scflow_pose_step_part's calls when the heads block is
// off (x NULL; drot NULL with parts = 1 is the given-pose form), scflow_pose_step_masked's
// otherwise; what only one entry refuses stays in that entry.
static int pose_step_launch(const scflow_pose_step_args& p, hipStream_t stream) {
  if (p.parts < 1 || p.parts > 3 || (!p.drot && (p.x || p.parts != 1))) return SCFLOW_EINVAL;
  if (p.x && (p.xsplit < 1 || !p.xbias || p.k <= 0 || !p.Wr || !p.br || !p.Wt || !p.bt ||
              !p.label || p.num_class <= 0 || !p.dt || p.rch != pose_rot_dim(p.depth_transform)))
    return SCFLOW_EINVAL;
  if ((p.mask_next || p.lrm_next) && !p.lr_next) return SCFLOW_EINVAL;
  if (p.lrm_next && (p.s_lrm < 2 || p.lrm_next == p.lr || p.lrm_next == p.lr_next))
    return SCFLOW_EINVAL;
  PoseStepArgs a;
  // (with the heads fused drot / dt are the outputs; the checks want a delta source: unread)
  const int st = pose_step_args(&a, p, 256);
  if (st != SCFLOW_OK) return st;
  if (!(p.parts & 1)) a.bf = 0;
  if (!(p.parts & 2)) a.bl = 0;
  if (a.bf + a.bl == 0) return SCFLOW_EINVAL;  // parts = 2 needs lr_next
  a.mnext = p.mask_next; a.o2 = p.lrm_next; a.s2 = p.s_lrm;
  if (p.x) {
    a.hx = p.x; a.hxs = (long long)p.n * p.k; a.hk = p.k; a.hsplit = p.xsplit; a.hxb = p.xbias;
    a.Wr = p.Wr; a.br = p.br; a.Wt = p.Wt; a.bt = p.bt; a.hlabel = p.label; a.hrch = p.rch;
    a.hncls = p.num_class; a.drot_out = p.drot; a.dt_out = p.dt;
  }
  pose_step_kernel<<<dim3(a.bf + a.bl, p.n), 256, 0, stream>>>(a);
  return scflow_launch_status();
}

SCFLOW_API int scflow_pose_step_call(const scflow_pose_step_args* args, void* stream) {
  return args ? pose_step_launch(*args, (hipStream_t)stream) : SCFLOW_EINVAL;
}

SCFLOW_API int scflow_pose_step(const float* drot6, const float* dt, const float* R_src,
                                const float* t_src, const float* K, const float* points,
                                float* R_dst, float* t_dst, float* flow, int n, int H, int W,
                                float weight, int depth_transform, float invalid_num,
                                const float* lr, const float* delta, const float* mask,
                                float* flow_up, float* mask_up, float* lr_next, int s_next,
                                float* hx_next, int s_hx, int h, int w, float up_scale,
                                float down_scale, void* stream) {
  if (!drot6) return SCFLOW_EINVAL;  // (only _part takes the given-pose form)
  return scflow_pose_step_part(drot6, dt, R_src, t_src, K, points, R_dst, t_dst, flow, n, H, W,
                               weight, depth_transform, invalid_num, lr, delta, mask, flow_up,
                               mask_up, lr_next, s_next, hx_next, s_hx, h, w, up_scale, down_scale,
                               3, stream);
}

SCFLOW_API int scflow_pose_step_part(const float* drot6, const float* dt, const float* R_src,
                                     const float* t_src, const float* K, const float* points,
                                     float* R_dst, float* t_dst, float* flow, int n, int H, int W,
                                     float weight, int depth_transform, float invalid_num,
                                     const float* lr, const float* delta, const float* mask,
                                     float* flow_up, float* mask_up, float* lr_next, int s_next,
                                     float* hx_next, int s_hx, int h, int w, float up_scale,
                                     float down_scale, int parts, void* stream) {
  scflow_pose_step_args p{};
  // (the struct's drot / dt are written only when the heads are fused: p.x stays NULL here)
  p.drot = const_cast<float*>(drot6); p.dt = const_cast<float*>(dt);
  p.R_src = R_src; p.t_src = t_src; p.K = K; p.points = points; p.R_dst = R_dst; p.t_dst = t_dst;
  p.flow = flow; p.n = n; p.H = H; p.W = W; p.weight = weight;
  p.depth_transform = depth_transform; p.invalid_num = invalid_num;
  p.lr = lr; p.delta = delta; p.mask = mask; p.flow_up = flow_up; p.mask_up = mask_up;
  p.h = h; p.w = w; p.up_scale = up_scale; p.down_scale = down_scale;
  p.lr_next = lr_next; p.s_next = s_next; p.hx_next = hx_next; p.s_hx = s_hx;
  p.parts = parts;
  return pose_step_launch(p, (hipStream_t)stream);
}

SCFLOW_API int scflow_pose_step_heads(const float* x, int xsplit, const float* xbias, int k,
                                      const float* Wr, const float* br, int rch, const float* Wt,
                                      const float* bt, const long long* label, int num_class,
                                      float* drot, float* dt, const float* R_src,
                                      const float* t_src, const float* K, const float* points,
                                      float* R_dst, float* t_dst, float* flow, int n, int H, int W,
                                      float weight, int depth_transform, float invalid_num,
                                      const float* lr, const float* delta, const float* mask,
                                      float* flow_up, float* mask_up, float* lr_next, int s_next,
                                      float* hx_next, int s_hx, int h, int w, float up_scale,
                                      float down_scale, int parts, void* stream) {
  if (!x) return SCFLOW_EINVAL;  // (the heads are this entry's point)
  return scflow_pose_step_masked(x, xsplit, xbias, k, Wr, br, rch, Wt, bt, label, num_class, drot,
                                 dt, R_src, t_src, K, points, R_dst, t_dst, flow, n, H, W, weight,
                                 depth_transform, invalid_num, lr, delta, mask, flow_up, mask_up,
                                 lr_next, s_next, hx_next, s_hx, nullptr, nullptr, 0, h, w,
                                 up_scale, down_scale, parts, stream);
}

// The superset of the three entries above with the masked tail: x NULL → scflow_pose_step_part
// (drot / dt read), else scflow_pose_step_heads (drot / dt written).  mask_next ([n·h·w], the mask
// this iteration just predicted) non-NULL: lr_next still receives the unmasked ↓8 flow; lrm_next
// (stride s_lrm, may be NULL) and hx_next receive lr_next · mask_next.  mask_next NULL: lrm_next,
// when given, is a copy of lr_next and everything else is the unmasked entry's, bit for bit.
SCFLOW_API int scflow_pose_step_masked(const float* x, int xsplit, const float* xbias, int k,
                                       const float* Wr, const float* br, int rch, const float* Wt,
                                       const float* bt, const long long* label, int num_class,
                                       float* drot, float* dt, const float* R_src,
                                       const float* t_src, const float* K, const float* points,
                                       float* R_dst, float* t_dst, float* flow, int n, int H, int W,
                                       float weight, int depth_transform, float invalid_num,
                                       const float* lr, const float* delta, const float* mask,
                                       float* flow_up, float* mask_up, float* lr_next, int s_next,
                                       float* hx_next, int s_hx, const float* mask_next,
                                       float* lrm_next, int s_lrm, int h, int w, float up_scale,
                                       float down_scale, int parts, void* stream) {
  if (!drot) return SCFLOW_EINVAL;  // (only _part takes the given-pose form)
  scflow_pose_step_args p{};
  p.x = x; p.xsplit = xsplit; p.xbias = xbias; p.k = k; p.Wr = Wr; p.br = br; p.rch = rch;
  p.Wt = Wt; p.bt = bt; p.label = label; p.num_class = num_class;
  p.drot = drot; p.dt = dt; p.R_src = R_src; p.t_src = t_src; p.K = K; p.points = points;
  p.R_dst = R_dst; p.t_dst = t_dst; p.flow = flow; p.n = n; p.H = H; p.W = W; p.weight = weight;
  p.depth_transform = depth_transform; p.invalid_num = invalid_num;
  p.lr = lr; p.delta = delta; p.mask = mask; p.flow_up = flow_up; p.mask_up = mask_up;
  p.h = h; p.w = w; p.up_scale = up_scale; p.down_scale = down_scale;
  p.lr_next = lr_next; p.s_next = s_next; p.hx_next = hx_next; p.s_hx = s_hx;
  p.mask_next = mask_next; p.lrm_next = lrm_next; p.s_lrm = s_lrm;
  p.parts = parts;
  return pose_step_launch(p, (hipStream_t)stream);
}

SCFLOW_API int scflow_transpose(const float* in, float* out, int n, int A, int B, long long ins,
                                int ias, long long ons, int obs, void* stream) {
  if (!in || !out || n <= 0 || A <= 0 || B <= 0 || ias < B || obs < A) return SCFLOW_EINVAL;
  dim3 grid(ceil_div(B, 32), ceil_div(A, 32), n);
  transpose_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(in, out, A, B, ins, ias, ons, obs);
  return scflow_launch_status();
}

SCFLOW_API int scflow_version(void) { return 1; }

SCFLOW_API const char* scflow_strerror(int code) {
  switch (code) {
    case SCFLOW_OK: return "ok";
    case SCFLOW_EINVAL: return "invalid argument";
    case SCFLOW_EUNSUPPORTED: return "unsupported shape for this build";
    case SCFLOW_EALIGN: return "pointer or stride not 16-byte aligned";
    default: return hipGetErrorString((hipError_t)code);
  }
}

// ------------------------------------------------------------------------------------------
// profiling helper: GPU wall-clock timestamps as graph-capturable kernel nodes
// ------------------------------------------------------------------------------------------
__global__ void timestamp_kernel(unsigned long long* stamps, int idx) {
  stamps[idx] = __builtin_amdgcn_s_memrealtime();
}

SCFLOW_API int scflow_timestamp(unsigned long long* stamps, int idx, void* stream) {
  if (!stamps || idx < 0) return SCFLOW_EINVAL;
  timestamp_kernel<<<1, 1, 0, (hipStream_t)stream>>>(stamps, idx);
  return scflow_launch_status();
}

SCFLOW_API long long scflow_wallclock_khz(void) {
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess) return SCFLOW_EINVAL;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return SCFLOW_EINVAL;
  return khz;
}
