// RAFT's convex upsampling (RAFTDecoder._upsample, raft_decoder.py:381-416; RAFTDecoderMask.
// upsample_flow / upsample_mask, raft_decoder_mask.py:104-160) as one launch: the softmax over the
// 3×3 neighbourhood of each of the 8×8 sub-pixels, the convex combination of the flow (and the
// occlusion, with the same weights) and the next iteration's low-resolution flow lr + delta.
//
// Mapping.  A workgroup (4 waves) owns a strip of 8 neighbouring low-resolution pixels of one row.
// A wave takes two of them, one after the other, with a lane per sub-pixel (lane = sy·8 + sx): the
// nine logits of a lane are channels k·64 + lane, so each of the nine loads of a wave is 256
// contiguous bytes.  The (8+2)×3 neighbourhood values lr + delta | occ of the strip are staged in
// LDS once (out-of-map neighbours as zeros, never loaded) and read back as wave-uniform
// broadcasts.  The results go through an LDS tile [channel][sy][8 pixels × 8 sx] so that the
// global stores are float4 runs along an output row (256 contiguous bytes per row and strip)
// instead of 32-byte fragments of eight rows per pixel.  The tile's rows are padded by 8 floats:
// a wave's 64 dword stores then fall on 32 distinct banks per half-wave.
#include "common.h"

namespace {

constexpr int kScale = 8;                      // sub-pixels per side
constexpr int kSub = kScale * kScale;          // lanes per low-resolution pixel
constexpr int kTaps = 9;                       // 3×3 neighbourhood
constexpr int kStrip = 8;                      // low-resolution pixels per workgroup
constexpr int kRow = kStrip * kScale + 8;      // floats per staged output row (padded)
constexpr int kLogits = kTaps * kSub;          // 576 channels

struct ConvexArgs {
  const float* logits;
  long long ls;
  const float* lr;
  const float* delta;
  const float* occ;
  float* flow_up;
  float* occ_up;
  float* next0;
  long long s0;
  float* next1;
  long long s1;
  int n, h, w;
  float logit_scale, value_scale;
};

// e^d for d ≤ 0 on the hardware exp2 with the argument's rounding compensated: d·log2(e) is
// split into the rounded product t and its residual r (the product's own rounding error plus the
// low part of log2 e), and 2^(t + r) = 2^t · (1 + r·ln 2) to first order.  Without the residual
// the result's relative error grows with |d| (|d| · 2^-24 · ln 2).
__device__ __forceinline__ float exp_neg(float d) {
  const float kHi = 1.44269504089f, kLo = 1.92596299e-8f;  // log2 e = kHi + kLo
  const float t = d * kHi;
  const float r = fmaf(d, kHi, -t) + d * kLo;
  const float e = __builtin_amdgcn_exp2f(t);
  return fmaf(e, r * 0.693147181f, e);
}

__global__ __launch_bounds__(256) void convex_upsample_kernel(ConvexArgs a) {
  __shared__ float nb[3][3][kStrip + 2];  // [fx | fy | occ][row y-1..y+1][column x0-1..x0+8]
  __shared__ __attribute__((aligned(16))) float stage[3][kScale][kRow];
  const int tid = threadIdx.x;
  const int strips = (a.w + kStrip - 1) / kStrip;
  int b = blockIdx.x;
  const int x0 = (b % strips) * kStrip;
  b /= strips;
  const int y = b % a.h;
  const int n = b / a.h;
  const int npx = a.w - x0 < kStrip ? a.w - x0 : kStrip;
  const long long row0 = ((long long)n * a.h + y) * a.w;  // pixel index of (n, y, 0)

  // this wave's logits first (nine coalesced loads per pixel), so that they are in flight while
  // the neighbourhood is staged
  const int wave = tid >> 6, lane = tid & 63;
  float lg[2][kTaps];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = wave * 2 + j;
    if (p < npx) {
      const float* src = a.logits + (row0 + x0 + p) * a.ls + lane;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) lg[j][k] = src[k * kSub];
    }
  }

  if (tid < 3 * (kStrip + 2)) {
    const int r = tid / (kStrip + 2), c = tid % (kStrip + 2);
    const int yy = y + r - 1, xx = x0 + c - 1;
    float fx = 0.f, fy = 0.f, oc = 0.f;
    if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) {
      const long long p = ((long long)n * a.h + yy) * a.w + xx;
      fx = a.lr[2 * p];
      fy = a.lr[2 * p + 1];
      if (a.delta) {
        fx += a.delta[2 * p];
        fy += a.delta[2 * p + 1];
      }
      if (a.occ) oc = a.occ[p];
      if (r == 1 && c >= 1 && c <= npx) {  // the strip's own pixels: the next iteration's flow
        if (a.next0) {
          a.next0[p * a.s0] = fx;
          a.next0[p * a.s0 + 1] = fy;
        }
        if (a.next1) {
          a.next1[p * a.s1] = fx;
          a.next1[p * a.s1 + 1] = fy;
        }
      }
    }
    nb[0][r][c] = fx;
    nb[1][r][c] = fy;
    nb[2][r][c] = oc;
  }
  __syncthreads();

  const int sy = lane >> 3, sx = lane & 7;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = wave * 2 + j;
    if (p < npx) {
      float m = lg[j][0];
#pragma unroll
      for (int k = 1; k < kTaps; ++k) m = fmaxf(m, lg[j][k]);
      float s = 0.f, ax = 0.f, ay = 0.f, ao = 0.f;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        // softmax(logit_scale · logits): the scaled values' maximum subtracted, as torch does
        const float e = exp_neg(a.logit_scale * lg[j][k] - a.logit_scale * m);
        const int ky = k / 3, kx = k % 3;
        s += e;
        ax = fmaf(e, nb[0][ky][p + kx], ax);
        ay = fmaf(e, nb[1][ky][p + kx], ay);
        ao = fmaf(e, nb[2][ky][p + kx], ao);
      }
      stage[0][sy][p * kScale + sx] = a.value_scale * (ax / s);
      stage[1][sy][p * kScale + sx] = a.value_scale * (ay / s);
      stage[2][sy][p * kScale + sx] = ao / s;
    }
  }
  __syncthreads();

  // [channel][sy] rows of npx·8 floats → float4 stores along the output rows
  const int H = a.h * kScale, W = a.w * kScale;
  const int rows = (a.occ ? 3 : 2) * kScale;
  for (int i = tid; i < rows * (kStrip * kScale / 4); i += 256) {
    const int row = i / (kStrip * kScale / 4), q = i % (kStrip * kScale / 4);
    if (q * 4 >= npx * kScale) continue;
    const int c = row / kScale, ry = row % kScale;
    const floatx4 v = *(const floatx4*)&stage[c][ry][q * 4];
    float* dst = c < 2 ? a.flow_up + ((size_t)n * 2 + c) * H * W : a.occ_up + (size_t)n * H * W;
    *(floatx4*)(dst + (size_t)(y * kScale + ry) * W + x0 * kScale + q * 4) = v;
  }
}

// ---------------------------------------------------------------------------------- backward
// The adjoint of the launch above, in two passes (no float atomics, a fixed summation order, so
// the result is bitwise reproducible).
//
// Pass 1 keeps the forward's mapping: a workgroup per strip of 8 pixels, a wave per two of them,
// a lane per sub-pixel.  The nine logits of a lane are the same nine coalesced 256-byte loads and
// the softmax is recomputed from them exactly as the forward computes it (exp_neg, the maximum
// subtracted); nothing is kept from the forward.  The incoming gradient rows of the strip are the
// forward's `stage` tile read the other way: float4 loads along the output rows into LDS, one
// dword per lane back out.  With dw_k = Σ_c vs_c · v_c[nb(p,k)] · g_c each lane writes its nine
// dlogits (the forward's access pattern), and the wave reduces the 9 × C products w_k · vs_c · g_c
// over its 64 lanes in a fixed order (wave_sum: DPP adds on the VALU; 9 × C butterflies through
// ds_bpermute kept the CU's one LDS pipe busy for most of the launch) into the table
// T[pixel][k][c].
//
// Pass 2 is a gather, one thread per low-resolution pixel q: dv_c[q] = Σ_k T[q − off(k)][k][c]
// over the in-map pixels, in order of k.
struct ConvexBwdArgs {
  const float* logits;
  long long ls;
  const float* x;
  const float* occ;
  const float* g_flow;
  const float* g_occ;
  float* dlogits;
  long long dls;
  float* table;
  int n, h, w;
  float logit_scale, value_scale;
};

template <int kCtrl, int kRowMask>
__device__ __forceinline__ float dpp_add(float v) {  // v + (v moved by the DPP control; 0 where masked)
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, kRowMask, 0xf,
                                                        false));
}

// Σ over the wave's 64 lanes on the VALU's DPP path (no LDS traffic), in a fixed order: within
// quads (lane^1, lane^2), within rows of 16 (rotations by 4 and 8), then row 0 → 1 and 2 → 3
// (row_bcast:15) and rows 0+1 → 3 (row_bcast:31).  Lane 63 holds the sum; it is returned
// wave-uniform.
__device__ __forceinline__ float wave_sum(float v) {
  v = dpp_add<0xb1, 0xf>(v);   // quad_perm:[1,0,3,2]
  v = dpp_add<0x4e, 0xf>(v);   // quad_perm:[2,3,0,1]
  v = dpp_add<0x124, 0xf>(v);  // row_ror:4
  v = dpp_add<0x128, 0xf>(v);  // row_ror:8
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

template <int C>  // 2: flow only; 3: flow + occlusion (occ and g_occ both given)
__global__ __launch_bounds__(256) void convex_upsample_bwd_kernel(ConvexBwdArgs a) {
  __shared__ float nb[3][3][kStrip + 2];
  __shared__ __attribute__((aligned(16))) float stage[3][kScale][kRow];
  const int tid = threadIdx.x;
  const int strips = (a.w + kStrip - 1) / kStrip;
  int b = blockIdx.x;
  const int x0 = (b % strips) * kStrip;
  b /= strips;
  const int y = b % a.h;
  const int n = b / a.h;
  const int npx = a.w - x0 < kStrip ? a.w - x0 : kStrip;
  const long long row0 = ((long long)n * a.h + y) * a.w;

  const int wave = tid >> 6, lane = tid & 63;
  float lg[2][kTaps];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = wave * 2 + j;
    if (p < npx) {
      const float* src = a.logits + (row0 + x0 + p) * a.ls + lane;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) lg[j][k] = src[k * kSub];
    }
  }

  // the strip's gradient rows: [channel][sy] rows of npx·8 floats, float4 along the output rows
  const int H = a.h * kScale, W = a.w * kScale;
  for (int i = tid; i < C * kScale * (kStrip * kScale / 4); i += 256) {
    const int row = i / (kStrip * kScale / 4), q = i % (kStrip * kScale / 4);
    if (q * 4 >= npx * kScale) continue;
    const int c = row / kScale, ry = row % kScale;
    const float* src = c < 2 ? a.g_flow + ((size_t)n * 2 + c) * H * W : a.g_occ + (size_t)n * H * W;
    *(floatx4*)&stage[c][ry][q * 4] =
        *(const floatx4*)(src + (size_t)(y * kScale + ry) * W + x0 * kScale + q * 4);
  }
  if (tid < 3 * (kStrip + 2)) {
    const int r = tid / (kStrip + 2), c = tid % (kStrip + 2);
    const int yy = y + r - 1, xx = x0 + c - 1;
    float fx = 0.f, fy = 0.f, oc = 0.f;
    if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) {
      const long long p = ((long long)n * a.h + yy) * a.w + xx;
      fx = a.x[2 * p];
      fy = a.x[2 * p + 1];
      if (C == 3) oc = a.occ[p];
    }
    nb[0][r][c] = fx;
    nb[1][r][c] = fy;
    nb[2][r][c] = oc;
  }
  __syncthreads();

  const int sy = lane >> 3, sx = lane & 7;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = wave * 2 + j;
    if (p >= npx) continue;  // wave-uniform
    float m = lg[j][0];
#pragma unroll
    for (int k = 1; k < kTaps; ++k) m = fmaxf(m, lg[j][k]);
    float e[kTaps], s = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      e[k] = exp_neg(a.logit_scale * lg[j][k] - a.logit_scale * m);
      s += e[k];
    }
    float g[3];
    g[0] = a.value_scale * stage[0][sy][p * kScale + sx];
    g[1] = a.value_scale * stage[1][sy][p * kScale + sx];
    g[2] = C == 3 ? stage[2][sy][p * kScale + sx] : 0.f;
    float wk[kTaps], dw[kTaps], dot = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const int ky = k / 3, kx = k % 3;
      wk[k] = e[k] / s;
      float d = g[0] * nb[0][ky][p + kx];
      d = fmaf(g[1], nb[1][ky][p + kx], d);
      if (C == 3) d = fmaf(g[2], nb[2][ky][p + kx], d);
      dw[k] = d;
      dot = fmaf(wk[k], d, dot);
    }
    float* dst = a.dlogits + (row0 + x0 + p) * a.dls + lane;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) dst[k * kSub] = a.logit_scale * wk[k] * (dw[k] - dot);

    // Σ over the 64 sub-pixels of w_k · vs_c · g_c; lane k·C + c keeps it for the store
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float t = wave_sum(wk[k] * g[c]);
        if (lane == k * C + c) mine = t;
      }
    }
    if (lane < kTaps * C) a.table[(row0 + x0 + p) * (kTaps * C) + lane] = mine;
  }
}

__global__ __launch_bounds__(256) void convex_upsample_gather_kernel(
    const float* __restrict__ table, int C, float* __restrict__ dx, float* __restrict__ docc, int h,
    int w, long long total) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= total) return;
  const int x = (int)(q % w), y = (int)((q / w) % h);
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < kTaps; ++k) {
    const int dy = k / 3 - 1, dxk = k % 3 - 1;  // nb(p, k) = p + (dy, dxk) = q
    const int py = y - dy, px = x - dxk;
    if (py < 0 || py >= h || px < 0 || px >= w) continue;
    const float* t = table + ((q - (long long)dy * w - dxk) * kTaps + k) * C;
    acc[0] += t[0];
    acc[1] += t[1];
    if (C == 3) acc[2] += t[2];
  }
  dx[2 * q] = acc[0];
  dx[2 * q + 1] = acc[1];
  if (docc) docc[q] = acc[2];
}

__global__ __launch_bounds__(256) void flow_add_kernel(const float* __restrict__ lr,
                                                       const float* __restrict__ delta,
                                                       float* out0, long long s0, float* out1,
                                                       long long s1, long long total) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const float fx = lr[2 * p] + delta[2 * p], fy = lr[2 * p + 1] + delta[2 * p + 1];
  out0[p * s0] = fx;
  out0[p * s0 + 1] = fy;
  if (out1) {
    out1[p * s1] = fx;
    out1[p * s1 + 1] = fy;
  }
}

}  // namespace

SCFLOW_API int scflow_convex_upsample(const float* logits, int ls, const float* lr,
                                      const float* delta, const float* occ, float* flow_up,
                                      float* occ_up, float* next0, int s0, float* next1, int s1,
                                      int n, int h, int w, int scale, int grid_side,
                                      float logit_scale, float value_scale, void* stream) {
  if (!logits || !lr || !flow_up || (occ && !occ_up) || n <= 0 || h <= 0 || w <= 0 ||
      scale <= 0 || grid_side <= 0 || (next0 && s0 < 2) || (next1 && s1 < 2))
    return SCFLOW_EINVAL;
  if (scale != kScale || grid_side != 3) return SCFLOW_EUNSUPPORTED;
  if (ls < kLogits) return SCFLOW_EINVAL;
  if (!aligned16(flow_up) || (occ && !aligned16(occ_up))) return SCFLOW_EALIGN;  // float4 stores
  const long long blocks = (long long)n * h * ((w + kStrip - 1) / kStrip);
  if (blocks > 0x7fffffffLL) return SCFLOW_EUNSUPPORTED;
  ConvexArgs a;
  a.logits = logits;
  a.ls = ls;
  a.lr = lr;
  a.delta = delta;
  a.occ = occ;
  a.flow_up = flow_up;
  a.occ_up = occ_up;
  a.next0 = next0;
  a.s0 = s0;
  a.next1 = next1;
  a.s1 = s1;
  a.n = n;
  a.h = h;
  a.w = w;
  a.logit_scale = logit_scale;
  a.value_scale = value_scale;
  convex_upsample_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a);
  return scflow_launch_status();
}

SCFLOW_API int scflow_convex_upsample_bwd(const float* logits, int ls, const float* x,
                                          const float* occ, const float* g_flow,
                                          const float* g_occ, float* dlogits, int dls, float* dx,
                                          float* docc, void* ws, long long ws_bytes, int n, int h,
                                          int w, int scale, int grid_side, float logit_scale,
                                          float value_scale, void* stream) {
  if (!logits || !x || !g_flow || !dlogits || !dx || !ws || (!occ && (g_occ || docc)) || n <= 0 ||
      h <= 0 || w <= 0 || scale <= 0 || grid_side <= 0)
    return SCFLOW_EINVAL;
  if (scale != kScale || grid_side != 3) return SCFLOW_EUNSUPPORTED;
  if (ls < kLogits || dls < kLogits) return SCFLOW_EINVAL;
  const int C = occ && g_occ ? 3 : 2;
  const long long total = (long long)n * h * w;
  if (ws_bytes < total * kTaps * C * (long long)sizeof(float)) return SCFLOW_EINVAL;
  if (!aligned16(g_flow) || (g_occ && !aligned16(g_occ))) return SCFLOW_EALIGN;  // float4 loads
  const long long blocks = (long long)n * h * ((w + kStrip - 1) / kStrip);
  if (blocks > 0x7fffffffLL || (total + 255) / 256 > 0x7fffffffLL) return SCFLOW_EUNSUPPORTED;
  ConvexBwdArgs a;
  a.logits = logits;
  a.ls = ls;
  a.x = x;
  a.occ = occ;
  a.g_flow = g_flow;
  a.g_occ = g_occ;
  a.dlogits = dlogits;
  a.dls = dls;
  a.table = (float*)ws;
  a.n = n;
  a.h = h;
  a.w = w;
  a.logit_scale = logit_scale;
  a.value_scale = value_scale;
  if (C == 3)
    convex_upsample_bwd_kernel<3><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a);
  else
    convex_upsample_bwd_kernel<2><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a);
  convex_upsample_gather_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (const float*)ws, C, dx, docc, h, w, total);
  return scflow_launch_status();
}

SCFLOW_API int scflow_flow_add(const float* lr, const float* delta, float* out0, int s0,
                               float* out1, int s1, int n, int h, int w, void* stream) {
  if (!lr || !delta || !out0 || s0 < 2 || (out1 && s1 < 2) || n <= 0 || h <= 0 || w <= 0)
    return SCFLOW_EINVAL;
  const long long total = (long long)n * h * w;
  flow_add_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      lr, delta, out0, s0, out1, s1, total);
  return scflow_launch_status();
}
