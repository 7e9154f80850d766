// Scene visibility (DESIGN.md §23 has the definitions): which instance is seen at each pixel of a
// frame, every instance's silhouette / valid / visible pixel counts and its two boxes, from the
// posed meshes of all instances of the frame and, optionally, the sensor depth.
//
//   scene_tile_kernel   one 256-lane workgroup owns one 16×16 tile of one frame's canvas (the
//                       frame plus its margins), one lane one pixel.  The frame's instances are a
//                       contiguous range of the non-decreasing frame_index (binary search); the
//                       workgroup walks those whose class bounding box (eight projected corners,
//                       one pixel of slack; every tile when a corner is at Z ≤ 0) meets the tile.
//                       A walked instance's faces are set up 256 at a time, one face per lane:
//                       three vertices posed and projected, dropped faces left out, the faces
//                       whose screen box meets the tile compacted into LDS; then every pixel tests
//                       the compacted faces and keeps the nearest depth.  The depths of up to
//                       kPlanes instances stay in LDS planes (lane-private columns), from which
//                       the test distance T, the visibility, the counters and inst_id follow.
//                       Counters and boxes are reduced per wave with one ballot per flag (a wave
//                       is four rows of sixteen pixels: the count is the mask's population, the
//                       box its occupied columns and rows), across waves through LDS, and leave
//                       the workgroup as one integer atomic per instance and non-zero counter.
//   A frame with more than kPlanes instances and no sensor depth is swept twice: T is the minimum
//   over all of them and must be known before the first count.
//
// Integer sums, minima and maxima only: the results do not depend on the order of anything.  Every
// output is computed by the same instructions whichever outputs are asked for (no template on
// them, contraction off), so an output asked for alone has the bits of the all-outputs call.
#include "common.h"

#include <limits.h>

namespace {

constexpr int ST = 16;       // tile side
constexpr int kPlanes = 32;  // instance depth planes a workgroup holds at a time (32 KB)
constexpr int kStats = 12;

__device__ __forceinline__ int lower_bound_scene(const int* __restrict__ v, int n, int key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// X = R·v + t, then (u, v) = (fx·X/Z + cx, fy·Y/Z + cy); returns Z
__device__ __forceinline__ float pose_project(const float* R, const float* t, float fx, float fy,
                                              float cx, float cy, float px, float py, float pz,
                                              float& u, float& v) {
  const float X = fmaf(R[2], pz, fmaf(R[1], py, fmaf(R[0], px, t[0])));
  const float Y = fmaf(R[5], pz, fmaf(R[4], py, fmaf(R[3], px, t[1])));
  const float Z = fmaf(R[8], pz, fmaf(R[7], py, fmaf(R[6], px, t[2])));
  u = fx * X / Z + cx;
  v = fy * Y / Z + cy;
  return Z;
}

// stats while the tiles accumulate: counts, then (x_min, y_min, x_max, y_max) of the two boxes
__global__ void scene_stats_init_kernel(int* __restrict__ stats, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int* s = stats + (size_t)i * kStats;
  s[0] = s[1] = s[2] = 0;
  s[3] = s[4] = INT_MAX;
  s[5] = s[6] = INT_MIN;
  s[7] = s[8] = INT_MAX;
  s[9] = s[10] = INT_MIN;
  s[11] = 0;
}

// (x_min, y_min, x_max, y_max) → (x, y, w, h); (−1, −1, −1, −1) for an empty box
__global__ void scene_stats_final_kernel(int* __restrict__ stats, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int* s = stats + (size_t)i * kStats;
  for (int b = 0; b < 2; ++b) {
    int* q = s + 3 + 4 * b;
    if (s[b == 0 ? 0 : 2] == 0) {
      q[0] = q[1] = q[2] = q[3] = -1;
    } else {
      q[2] = q[2] - q[0] + 1;
      q[3] = q[3] - q[1] + 1;
    }
  }
}

__global__ __launch_bounds__(256) void scene_tile_kernel(scflow_scene_args a) {
#pragma clang fp contract(off)
  __shared__ float planes[kPlanes][256];
  __shared__ float lf[256][9];  // x0 y0 x1 y1 x2 y2 1/Z0 1/Z1 1/Z2, counter-clockwise in (x, y)
  __shared__ int list[256];
  __shared__ int red[4][kPlanes][5];
  __shared__ int range[2];
  __shared__ int cnt, lcnt;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = blockIdx.y;
  const int W = a.width, H = a.height;
  const int tiles_x = (W + 2 * a.margin_x + ST - 1) / ST;
  const int tx0 = (int)(blockIdx.x % tiles_x) * ST - a.margin_x;
  const int ty0 = (int)(blockIdx.x / tiles_x) * ST - a.margin_y;
  const int x = tx0 + (tid & 15), y = ty0 + (tid >> 4);
  const bool in_canvas = x < W + a.margin_x && y < H + a.margin_y;
  const bool in_frame = x >= 0 && y >= 0 && x < W && y < H;
  // a tile outside the frame only feeds px_count_all and bbox_obj
  const bool tile_in_frame = tx0 + ST > 0 && ty0 + ST > 0 && tx0 < W && ty0 < H;
  if (!tile_in_frame && !a.stats) return;

  if (tid < 2) range[tid] = lower_bound_scene(a.frame_index, a.n, f + tid);
  const float fx = a.K[(size_t)f * 9], cx = a.K[(size_t)f * 9 + 2];
  const float fy = a.K[(size_t)f * 9 + 4], cy = a.K[(size_t)f * 9 + 5];
  const float sx = (float)x + a.pixel_offset, sy = (float)y + a.pixel_offset;
  // the tile's sample range
  const float slo_x = (float)tx0 + a.pixel_offset, shi_x = (float)(tx0 + ST - 1) + a.pixel_offset;
  const float slo_y = (float)ty0 + a.pixel_offset, shi_y = (float)(ty0 + ST - 1) + a.pixel_offset;
  // depth → distance from the camera centre (scflow_vsd_counts' factor)
  const float ax = ((float)x - cx) * (1.f / fx), ay = ((float)y - cy) * (1.f / fy);
  const float dist = sqrtf(fmaf(ax, ax, fmaf(ay, ay, 1.f)));
  const float inf = __int_as_float(0x7f800000);
  const size_t pix = in_frame ? (size_t)y * W + x : 0;
  const float* __restrict__ dt = a.depth_test;
  const float T_sensor = (dt && in_frame) ? dt[(size_t)f * H * W + pix] * dist : 0.f;
  __syncthreads();
  const int ib = range[0], ie = range[1];

  const bool tsweep = !dt && ie - ib > kPlanes;
  float d_first = inf;   // sweep 0: the nearest depth over all instances
  float d_scene = inf;   // sweep 1: the same, for depth_scene
  float best_m = inf;
  int best_i = -1;

  for (int sweep = tsweep ? 0 : 1; sweep < 2; ++sweep) {
    for (int c0 = ib; c0 < ie; c0 += 256) {
      // ---- the instances of this chunk whose class box meets the tile
      __syncthreads();
      if (tid == 0) lcnt = 0;
      __syncthreads();
      const int ci = c0 + tid;
      if (ci < ie) {
        const int lab = a.labels[ci];
        bool walk = lab >= 0 && lab < a.num_classes;
        if (walk) {
          const int v0 = max(a.vert_offset[lab], 0), v1 = min(a.vert_offset[lab + 1], a.total_verts);
          const int f0 = max(a.face_offset[lab], 0), f1 = min(a.face_offset[lab + 1], a.total_faces);
          walk = v1 > v0 && f1 > f0;
        }
        if (walk) {
          const float* __restrict__ R = a.R + (size_t)ci * 9;
          const float* __restrict__ t = a.t + (size_t)ci * 3;
          const float* __restrict__ bb = a.bounds + (size_t)lab * 6;
          float Rr[9], tt[3];
          for (int e = 0; e < 9; ++e) Rr[e] = R[e];
          for (int e = 0; e < 3; ++e) tt[e] = t[e];
          bool behind = false;
          float umin = inf, umax = -inf, vmin = inf, vmax = -inf;
          for (int c = 0; c < 8; ++c) {
            float u, v;
            const float Z = pose_project(Rr, tt, fx, fy, cx, cy, bb[(c & 1) ? 3 : 0],
                                         bb[(c & 2) ? 4 : 1], bb[(c & 4) ? 5 : 2], u, v);
            behind = behind || !(Z > 0.f);
            umin = fminf(umin, u), umax = fmaxf(umax, u);
            vmin = fminf(vmin, v), vmax = fmaxf(vmax, v);
          }
          // one pixel of slack for the rounding of the corners against that of the vertices
          walk = behind || (!(umax + 1.f < slo_x) && !(umin - 1.f > shi_x) &&
                            !(vmax + 1.f < slo_y) && !(vmin - 1.f > shi_y));
        }
        if (walk) list[atomicAdd(&lcnt, 1)] = ci;
      }
      __syncthreads();
      const int m = lcnt;

      for (int p0 = 0; p0 < m; p0 += kPlanes) {
        const int np = min(kPlanes, m - p0);
        // ---- rasterise np instances into the planes
        for (int k = 0; k < np; ++k) {
          const int i = __builtin_amdgcn_readfirstlane(list[p0 + k]);
          const int lab = a.labels[i];
          const int v0 = max(a.vert_offset[lab], 0), v1 = min(a.vert_offset[lab + 1], a.total_verts);
          const int fb = max(a.face_offset[lab], 0), fe = min(a.face_offset[lab + 1], a.total_faces);
          const int nv = v1 - v0;
          float Rr[9], tt[3];
          for (int e = 0; e < 9; ++e) Rr[e] = a.R[(size_t)i * 9 + e];
          for (int e = 0; e < 3; ++e) tt[e] = a.t[(size_t)i * 3 + e];
          const float* __restrict__ verts = a.verts + (size_t)v0 * 3;
          float d = inf;
          for (int fc = fb; fc < fe; fc += 256) {
            __syncthreads();  // the previous list has been read
            if (tid == 0) cnt = 0;
            __syncthreads();
            const int fi = fc + tid;
            if (fi < fe) {
              const int j0 = a.faces[(size_t)fi * 3], j1 = a.faces[(size_t)fi * 3 + 1],
                        j2 = a.faces[(size_t)fi * 3 + 2];
              // an index outside the class's block: the face is dropped, nothing is read
              if (j0 >= 0 && j0 < nv && j1 >= 0 && j1 < nv && j2 >= 0 && j2 < nv) {
                float x0, y0, x1, y1, x2, y2;
                const float Z0 = pose_project(Rr, tt, fx, fy, cx, cy, verts[j0 * 3], verts[j0 * 3 + 1],
                                              verts[j0 * 3 + 2], x0, y0);
                float Z1 = pose_project(Rr, tt, fx, fy, cx, cy, verts[j1 * 3], verts[j1 * 3 + 1],
                                        verts[j1 * 3 + 2], x1, y1);
                float Z2 = pose_project(Rr, tt, fx, fy, cx, cy, verts[j2 * 3], verts[j2 * 3 + 1],
                                        verts[j2 * 3 + 2], x2, y2);
                if (Z0 > 0.f && Z1 > 0.f && Z2 > 0.f) {
                  const float area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
                  const float umin = fminf(x0, fminf(x1, x2)), umax = fmaxf(x0, fmaxf(x1, x2));
                  const float vmin = fminf(y0, fminf(y1, y2)), vmax = fmaxf(y0, fmaxf(y1, y2));
                  // a sample outside the face's box has an edge function ≤ 0: nothing is lost
                  if ((area > 0.f || area < 0.f) && umax >= slo_x && umin <= shi_x &&
                      vmax >= slo_y && vmin <= shi_y) {
                    if (area < 0.f) {
                      float s;
                      s = x1, x1 = x2, x2 = s;
                      s = y1, y1 = y2, y2 = s;
                      s = Z1, Z1 = Z2, Z2 = s;
                    }
                    float* q = lf[atomicAdd(&cnt, 1)];
                    q[0] = x0, q[1] = y0, q[2] = x1, q[3] = y1, q[4] = x2, q[5] = y2;
                    q[6] = 1.f / Z0, q[7] = 1.f / Z1, q[8] = 1.f / Z2;
                  }
                }
              }
            }
            __syncthreads();
            const int nf = cnt;
            if (in_canvas)
              for (int q = 0; q < nf; ++q) {
                const float ax0 = lf[q][0] - sx, ay0 = lf[q][1] - sy;
                const float ax1 = lf[q][2] - sx, ay1 = lf[q][3] - sy;
                const float ax2 = lf[q][4] - sx, ay2 = lf[q][5] - sy;
                // plain products: the two faces of a shared edge get negated values, never both > 0
                const float e0 = ax1 * ay2 - ay1 * ax2;
                const float e1 = ax2 * ay0 - ay2 * ax0;
                const float e2 = ax0 * ay1 - ay0 * ax1;
                if (e0 > 0.f && e1 > 0.f && e2 > 0.f) {
                  // 1 / Σ w_i/Z_i with w_i = e_i / Σ e: inside the face's depth range whatever the
                  // rounding of the weights
                  const float z = (e0 + e1 + e2) / (e0 * lf[q][6] + e1 * lf[q][7] + e2 * lf[q][8]);
                  d = fminf(d, z);
                }
              }
          }
          planes[k][tid] = d;  // a lane reads only its own column: no barrier
        }

        if (sweep == 0) {
          for (int k = 0; k < np; ++k) d_first = fminf(d_first, planes[k][tid]);
          continue;
        }
        // ---- the test distance
        float T = T_sensor;
        if (!dt) {
          float dn = d_first;
          if (!tsweep)
            for (int k = 0; k < np; ++k) dn = fminf(dn, planes[k][tid]);
          T = dn < inf ? dn * dist : 0.f;
        }
        // ---- visibility, counters, maps
        for (int k = 0; k < np; ++k) {
          const int i = __builtin_amdgcn_readfirstlane(list[p0 + k]);
          const float d = planes[k][tid];
          const bool cov = d < inf;  // in_canvas holds: other lanes never rasterise
          const bool covf = cov && in_frame;
          const float M = d * dist;
          const bool vis = covf && (T == 0.f || M - T <= a.delta);
          if (covf) {
            d_scene = fminf(d_scene, d);
            if (vis && (M < best_m || (M == best_m && i < best_i))) best_m = M, best_i = i;
            if (a.depth_inst) a.depth_inst[(size_t)i * H * W + pix] = d;
            if (vis && a.mask_visib) a.mask_visib[(size_t)i * H * W + pix] = 1;
          }
          if (a.stats) {
            const unsigned long long b_all = __ballot(cov);
            const unsigned long long b_val = __ballot(covf && T > 0.f);
            const unsigned long long b_vis = __ballot(vis);
            if (lane == 0) {
              int* r = red[wave][k];
              r[0] = __popcll(b_all);
              r[1] = __popcll(b_val);
              r[2] = __popcll(b_vis);
#pragma unroll
              for (int w = 0; w < 2; ++w) {
                const unsigned long long b = w ? b_vis : b_all;
                const unsigned cols = (unsigned)((b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xffffu);
                const unsigned rows = ((b & 0xffffull) ? 1u : 0u) | (((b >> 16) & 0xffffull) ? 2u : 0u) |
                                      (((b >> 32) & 0xffffull) ? 4u : 0u) | ((b >> 48) ? 8u : 0u);
                r[3 + w] = (int)(cols | (rows << 16));
              }
            }
          }
        }
        if (a.stats) {
          __syncthreads();
          if (tid < np) {
            const int i = list[p0 + tid];
            int* s = a.stats + (size_t)i * kStats;
            int c[3] = {0, 0, 0};
            unsigned cols[2] = {0, 0}, rows[2] = {0, 0};
            for (int w = 0; w < 4; ++w) {
              const int* r = red[w][tid];
              c[0] += r[0], c[1] += r[1], c[2] += r[2];
              for (int b = 0; b < 2; ++b) {
                cols[b] |= (unsigned)r[3 + b] & 0xffffu;
                rows[b] |= (((unsigned)r[3 + b] >> 16) & 0xfu) << (4 * w);
              }
            }
            if (c[0]) atomicAdd(s, c[0]);
            if (c[1]) atomicAdd(s + 1, c[1]);
            if (c[2]) atomicAdd(s + 2, c[2]);
            for (int b = 0; b < 2; ++b)
              if (cols[b]) {
                int* q = s + 3 + 4 * b;
                atomicMin(q, tx0 + __builtin_ctz(cols[b]));
                atomicMin(q + 1, ty0 + __builtin_ctz(rows[b]));
                atomicMax(q + 2, tx0 + 31 - __builtin_clz(cols[b]));
                atomicMax(q + 3, ty0 + 31 - __builtin_clz(rows[b]));
              }
          }
          __syncthreads();  // red is rewritten by the next pass
        }
      }
    }
  }

  if (in_frame) {
    if (a.inst_id) a.inst_id[(size_t)f * H * W + pix] = best_i;
    if (a.depth_scene) a.depth_scene[(size_t)f * H * W + pix] = d_scene < inf ? d_scene : 0.f;
  }
}

}  // namespace

SCFLOW_API int scflow_scene_visibility(const scflow_scene_args* args, void* stream) {
  if (!args) return SCFLOW_EINVAL;
  const scflow_scene_args a = *args;
  if (!a.verts || !a.faces || !a.vert_offset || !a.face_offset || !a.bounds || !a.labels ||
      !a.frame_index || !a.R || !a.t || !a.K || a.num_classes < 1 || a.total_verts < 1 ||
      a.total_faces < 1 || a.n < 0 || a.n_frames < 1 || a.height < 1 || a.width < 1 ||
      a.margin_x < 0 || a.margin_y < 0 || !(a.delta >= 0.f) ||
      (!a.stats && !a.inst_id && !a.depth_scene && !a.depth_inst && !a.mask_visib))
    return SCFLOW_EINVAL;
  if (a.n == 0) return SCFLOW_OK;
  const long long Wc = (long long)a.width + 2LL * a.margin_x, Hc = (long long)a.height + 2LL * a.margin_y;
  const long long tiles = ((Wc + ST - 1) / ST) * ((Hc + ST - 1) / ST);
  if (Wc > (1LL << 24) || Hc > (1LL << 24) || tiles > INT_MAX || a.n_frames > 65535)
    return SCFLOW_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const size_t hw = (size_t)a.height * a.width;
  hipError_t e = hipSuccess;
  // the tiles write the per-instance planes only where an instance is: the rest is 0
  if (a.depth_inst) e = hipMemsetAsync(a.depth_inst, 0, (size_t)a.n * hw * sizeof(float), st);
  if (e == hipSuccess && a.mask_visib) e = hipMemsetAsync(a.mask_visib, 0, (size_t)a.n * hw, st);
  if (e != hipSuccess) return (int)e;
  if (a.stats) scene_stats_init_kernel<<<ceil_div(a.n, 256), 256, 0, st>>>(a.stats, a.n);
  scene_tile_kernel<<<dim3((unsigned)tiles, a.n_frames), 256, 0, st>>>(a);
  if (a.stats) scene_stats_final_kernel<<<ceil_div(a.n, 256), 256, 0, st>>>(a.stats, a.n);
  return scflow_launch_status();
}
