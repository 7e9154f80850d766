// Batched RANSAC-PnP: the pose half of the RAFT + PnP baseline.
//
//   solve_pose                     /root/reference/models/refiner/base_flow_refiner.py:99-155
//   get_2d_3d_corr_by_fw_flow      /root/reference/models/utils/pose.py:182-200
//   solve_pose_by_pnp              /root/reference/models/utils/pose.py:203-249 (cv2.solvePnPRansac)
//
// The reference enumerates the foreground pixels per sample on the host and hands them to cv2 behind
// .cpu().numpy().  Here the whole batch stays on the device, on the caller's stream, in five
// launches with no host synchronisation (DESIGN.md §14 has the contract):
//   compact    ordered stream compaction of the valid pixels' (X, Y, Z, u, v) — per-chunk counts,
//              then a scan; the order is the pixel order, never the arrival order
//   hypotheses one thread per (sample, hypothesis): four hashed indices, Grunert's P3P in fp64
//              (quartic by Ferrari + Newton), the root that reprojects the fourth point best
//   score      the hot kernel: every point against every hypothesis, hypotheses broadcast from LDS,
//              wave ballots + popcounts into LDS counters, one integer add per hypothesis and
//              workgroup to global memory
//   refine     one workgroup per sample: winner (highest score, lowest index), then Gauss-Newton on
//              its inlier set — residuals, Jacobians and the normal equations in fp64, a fixed
//              reduction order, Cholesky in fp64
// Integer sums only cross lanes and workgroups out of order; there is no floating-point atomic.
#include "common.h"

namespace {

constexpr int kChunk = 1024;  // pixels per compaction workgroup and points per scoring workgroup
constexpr double kCollinearSin2 = 1e-4;

__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// ------------------------------------------------------------------------------- compaction
// validity of the calling thread's four consecutive pixels (bit j: pixel p0 + j)
__device__ __forceinline__ int valid_bits(const floatx4* __restrict__ pts,
                                          const float* __restrict__ mask, size_t base, int p0,
                                          int HW) {
  int bits = 0;
  for (int j = 0; j < 4; ++j) {
    const int p = p0 + j;
    if (p < HW && pts[base + p][3] > 0.f && (!mask || mask[base + p] != 0.f)) bits |= 1 << j;
  }
  return bits;
}

// exclusive prefix of c over the 256 threads of the workgroup (thread order) and the total
__device__ __forceinline__ int block_scan(int c, int* sh, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = c;
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d);
    if (lane >= d) incl += v;
  }
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
  for (int i = 0; i < 4; ++i) {
    if (i < wave) before += sh[i];
    total += sh[i];
  }
  return before + incl - c;
}

__global__ __launch_bounds__(256) void compact_count_kernel(const floatx4* __restrict__ pts,
                                                            const float* __restrict__ mask,
                                                            int* __restrict__ chunk_cnt, int HW) {
  __shared__ int sh[4];
  const int b = blockIdx.y;
  const int bits = valid_bits(pts, mask, (size_t)b * HW, blockIdx.x * kChunk + threadIdx.x * 4, HW);
  int total;
  block_scan(__popc(bits), sh, total);
  if (threadIdx.x == 0) chunk_cnt[b * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void compact_write_kernel(const floatx4* __restrict__ pts,
                                                            const float* __restrict__ flow,
                                                            const float* __restrict__ mask,
                                                            const int* __restrict__ chunk_cnt,
                                                            float* __restrict__ corr,
                                                            int* __restrict__ count, int HW, int W) {
  __shared__ int sh[4];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * HW;
  const int p0 = blockIdx.x * kChunk + threadIdx.x * 4;
  const int bits = valid_bits(pts, mask, base, p0, HW);
  int total;
  int row = block_scan(__popc(bits), sh, total);
  for (int i = 0; i < (int)blockIdx.x; ++i) row += chunk_cnt[b * gridDim.x + i];
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) count[b] = row + __popc(bits);
  for (int j = 0; j < 4; ++j) {
    if (!(bits >> j & 1)) continue;
    const int p = p0 + j;
    const floatx4 P = pts[base + p];
    float* o = corr + (base + row) * 5;  // row < number of valid pixels ≤ HW
    o[0] = P[0];
    o[1] = P[1];
    o[2] = P[2];
    o[3] = (float)(p % W) + flow[(size_t)b * 2 * HW + p];
    o[4] = (float)(p / W) + flow[((size_t)b * 2 + 1) * HW + p];
    ++row;
  }
}

// ------------------------------------------------------------------------------- hypotheses
__device__ __forceinline__ double dot3(const double* a, const double* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.79769313486231570e308; }

// real roots of c4 v⁴ + c3 v³ + c2 v² + c1 v + c0 (c4 ≠ 0): Ferrari through the largest real root of
// the resolvent cubic, two quadratics, then Newton on the quartic itself
__device__ int solve_quartic(const double* c, double* roots) {
  const double a = c[1] / c[0], b = c[2] / c[0], cc = c[3] / c[0], d = c[4] / c[0];
  const double a2 = a * a;
  const double p = b - 0.375 * a2;
  const double q = cc - 0.5 * a * b + 0.125 * a2 * a;
  const double r = d - 0.25 * a * cc + 0.0625 * a2 * b - (3.0 / 256.0) * a2 * a2;
  double y[4];
  int n = 0;
  // resolvent m³ + B m² + C m + D = 0
  const double B = p, C = 0.25 * (p * p - 4.0 * r), D = -0.125 * q * q;
  const double P3 = C - B * B / 3.0, Q3 = 2.0 * B * B * B / 27.0 - B * C / 3.0 + D;
  const double disc = 0.25 * Q3 * Q3 + P3 * P3 * P3 / 27.0;
  double w;
  if (disc > 0.0) {
    const double sd = sqrt(disc);
    w = cbrt(-0.5 * Q3 + sd) + cbrt(-0.5 * Q3 - sd);
  } else if (P3 < 0.0) {
    double arg = 1.5 * Q3 / P3 * sqrt(-3.0 / P3);
    arg = arg < -1.0 ? -1.0 : (arg > 1.0 ? 1.0 : arg);
    w = 2.0 * sqrt(-P3 / 3.0) * cos(acos(arg) / 3.0);
  } else {
    w = 0.0;
  }
  double m = w - B / 3.0;
  for (int it = 0; it < 3; ++it) {
    const double f = ((m + B) * m + C) * m + D, fp = (3.0 * m + 2.0 * B) * m + C;
    if (fp != 0.0 && finite_d(f / fp)) m -= f / fp;
  }
  const double s = m > 0.0 ? sqrt(2.0 * m) : 0.0;
  if (s > 0.0 && finite_d(q / s)) {
    const double h = 0.5 * p + m, g = 0.5 * q / s;
    const double d1 = s * s - 4.0 * (h + g), d2 = s * s - 4.0 * (h - g);
    if (d1 >= 0.0) {
      y[n++] = 0.5 * (s + sqrt(d1));
      y[n++] = 0.5 * (s - sqrt(d1));
    }
    if (d2 >= 0.0) {
      y[n++] = 0.5 * (-s + sqrt(d2));
      y[n++] = 0.5 * (-s - sqrt(d2));
    }
  } else {  // q = 0: biquadratic in y
    const double dd = p * p - 4.0 * r;
    if (dd >= 0.0) {
      const double z1 = 0.5 * (-p + sqrt(dd)), z2 = 0.5 * (-p - sqrt(dd));
      if (z1 >= 0.0) {
        y[n++] = sqrt(z1);
        y[n++] = -sqrt(z1);
      }
      if (z2 >= 0.0) {
        y[n++] = sqrt(z2);
        y[n++] = -sqrt(z2);
      }
    }
  }
  for (int i = 0; i < n; ++i) {
    double v = y[i] - 0.25 * a;
    for (int it = 0; it < 3; ++it) {
      const double f = (((c[0] * v + c[1]) * v + c[2]) * v + c[3]) * v + c[4];
      const double fp = ((4.0 * c[0] * v + 3.0 * c[1]) * v + 2.0 * c[2]) * v + c[3];
      if (fp != 0.0 && finite_d(f / fp)) v -= f / fp;
    }
    roots[i] = v;
  }
  return n;
}

// Grunert's P3P on points 0..2, the root chosen by point 3.  X [4][3], uv [4][2]; K, Kinv row-major.
__device__ bool p3p_best(const double (*X)[3], const double (*uv)[2], const double* K,
                         const double* Kinv, double* Rb, double* tb) {
  double d1[3], d2[3], d12[3], cr[3];
  for (int i = 0; i < 3; ++i) {
    d1[i] = X[1][i] - X[0][i];
    d2[i] = X[2][i] - X[0][i];
    d12[i] = X[1][i] - X[2][i];
  }
  cross3(d1, d2, cr);
  const double c2 = dot3(d1, d1), b2 = dot3(d2, d2), a2 = dot3(d12, d12);
  if (!(dot3(cr, cr) > kCollinearSin2 * c2 * b2)) return false;
  double j[3][3];
  for (int i = 0; i < 3; ++i) {
    double v[3];
    for (int r = 0; r < 3; ++r) v[r] = Kinv[r * 3] * uv[i][0] + Kinv[r * 3 + 1] * uv[i][1] + Kinv[r * 3 + 2];
    const double inv = 1.0 / sqrt(dot3(v, v));
    for (int r = 0; r < 3; ++r) j[i][r] = v[r] * inv;
  }
  const double ca = dot3(j[1], j[2]), cb = dot3(j[0], j[2]), cg = dot3(j[0], j[1]);
  const double k = (a2 - c2) / b2, q = c2 / b2;
  // u = N(v) / D(v);  quartic N² + D²·W − 2cg·N·D = 0
  const double n2 = k - 1.0, n1 = -2.0 * k * cb, n0 = 1.0 + k;
  const double e1 = -2.0 * ca, e0 = 2.0 * cg;
  const double w2 = -q, w1 = 2.0 * q * cb, w0 = 1.0 - q;
  const double D2 = e1 * e1, D1 = 2.0 * e1 * e0, D0 = e0 * e0;
  double c[5];
  c[0] = n2 * n2 + D2 * w2;
  c[1] = 2.0 * n2 * n1 + D2 * w1 + D1 * w2 - 2.0 * cg * (n2 * e1);
  c[2] = 2.0 * n2 * n0 + n1 * n1 + D2 * w0 + D1 * w1 + D0 * w2 - 2.0 * cg * (n2 * e0 + n1 * e1);
  c[3] = 2.0 * n1 * n0 + D1 * w0 + D0 * w1 - 2.0 * cg * (n1 * e0 + n0 * e1);
  c[4] = n0 * n0 + D0 * w0 - 2.0 * cg * (n0 * e0);
  for (int i = 0; i < 5; ++i)
    if (!finite_d(c[i])) return false;
  if (c[0] == 0.0) return false;
  double roots[4];
  const int nr = solve_quartic(c, roots);
  // object-space frame of the triangle
  double E[3][3];
  {
    const double i1 = 1.0 / sqrt(c2), i3 = 1.0 / sqrt(dot3(cr, cr));
    for (int i = 0; i < 3; ++i) {
      E[0][i] = d1[i] * i1;
      E[2][i] = cr[i] * i3;
    }
    cross3(E[2], E[0], E[1]);
  }
  double best = -1.0;
  for (int ir = 0; ir < nr; ++ir) {
    const double v = roots[ir];
    if (!(v > 0.0) || !finite_d(v)) continue;
    const double den = e1 * v + e0;
    if (den == 0.0) continue;
    const double u = ((n2 * v + n1) * v + n0) / den;
    const double s0sq = b2 / (1.0 + v * v - 2.0 * v * cb);
    if (!(u > 0.0) || !(s0sq > 0.0) || !finite_d(u) || !finite_d(s0sq)) continue;
    const double s0 = sqrt(s0sq), s[3] = {s0, u * s0, v * s0};
    double Q[3][3], g1[3], g2[3], F[3][3], gc[3];
    for (int i = 0; i < 3; ++i)
      for (int r = 0; r < 3; ++r) Q[i][r] = j[i][r] * s[i];
    for (int r = 0; r < 3; ++r) {
      g1[r] = Q[1][r] - Q[0][r];
      g2[r] = Q[2][r] - Q[0][r];
    }
    cross3(g1, g2, gc);
    const double l1 = dot3(g1, g1), l3 = dot3(gc, gc);
    if (!(l1 > 0.0) || !(l3 > 0.0)) continue;
    const double i1 = 1.0 / sqrt(l1), i3 = 1.0 / sqrt(l3);
    for (int r = 0; r < 3; ++r) {
      F[0][r] = g1[r] * i1;
      F[2][r] = gc[r] * i3;
    }
    cross3(F[2], F[0], F[1]);
    double R[9], t[3];
    bool fin = true;
    for (int r = 0; r < 3; ++r)
      for (int cidx = 0; cidx < 3; ++cidx)
        R[r * 3 + cidx] = F[0][r] * E[0][cidx] + F[1][r] * E[1][cidx] + F[2][r] * E[2][cidx];
    for (int r = 0; r < 3; ++r) {
      t[r] = Q[0][r] - (R[r * 3] * X[0][0] + R[r * 3 + 1] * X[0][1] + R[r * 3 + 2] * X[0][2]);
      fin = fin && finite_d(t[r]);
    }
    for (int i = 0; i < 9; ++i) fin = fin && finite_d(R[i]);
    if (!fin) continue;
    double xc[3], pr[3];
    for (int r = 0; r < 3; ++r)
      xc[r] = R[r * 3] * X[3][0] + R[r * 3 + 1] * X[3][1] + R[r * 3 + 2] * X[3][2] + t[r];
    if (!(xc[2] > 0.0)) continue;
    for (int r = 0; r < 3; ++r) pr[r] = K[r * 3] * xc[0] + K[r * 3 + 1] * xc[1] + K[r * 3 + 2] * xc[2];
    const double ex = pr[0] / pr[2] - uv[3][0], ey = pr[1] / pr[2] - uv[3][1];
    const double e = sqrt(ex * ex + ey * ey);
    if (!finite_d(e)) continue;
    if (best < 0.0 || e < best) {
      best = e;
      for (int i = 0; i < 9; ++i) Rb[i] = R[i];
      for (int i = 0; i < 3; ++i) tb[i] = t[i];
    }
  }
  return best >= 0.0;
}

__global__ __launch_bounds__(64) void hypotheses_kernel(const float* __restrict__ corr,
                                                        const int* __restrict__ count,
                                                        const float* __restrict__ Kf,
                                                        float* __restrict__ hyp,
                                                        float* __restrict__ hyp_rt,
                                                        int* __restrict__ hyp_valid,
                                                        int* __restrict__ samples, int n, int HW,
                                                        int hyps, uint32_t seed) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n * hyps) return;
  const int b = i / hyps;
  const int cnt = count[b];
  int s[4];
  for (int k = 0; k < 4; ++k)
    s[k] = (int)(((uint64_t)lowbias32(((uint32_t)i * 4u + (uint32_t)k) ^ seed) * (uint64_t)(uint32_t)cnt) >> 32);
  if (samples)
    for (int k = 0; k < 4; ++k) samples[(size_t)i * 4 + k] = s[k];
  bool ok = cnt >= 4 && cnt <= HW && s[0] != s[1] && s[0] != s[2] && s[0] != s[3] && s[1] != s[2] &&
            s[1] != s[3] && s[2] != s[3];
  double K[9], Kinv[9], R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  if (ok) {
    for (int k = 0; k < 9; ++k) K[k] = (double)Kf[b * 9 + k];
    const double det = K[0] * (K[4] * K[8] - K[5] * K[7]) - K[1] * (K[3] * K[8] - K[5] * K[6]) +
                       K[2] * (K[3] * K[7] - K[4] * K[6]);
    const double id = 1.0 / det;
    Kinv[0] = (K[4] * K[8] - K[5] * K[7]) * id;
    Kinv[1] = (K[2] * K[7] - K[1] * K[8]) * id;
    Kinv[2] = (K[1] * K[5] - K[2] * K[4]) * id;
    Kinv[3] = (K[5] * K[6] - K[3] * K[8]) * id;
    Kinv[4] = (K[0] * K[8] - K[2] * K[6]) * id;
    Kinv[5] = (K[2] * K[3] - K[0] * K[5]) * id;
    Kinv[6] = (K[3] * K[7] - K[4] * K[6]) * id;
    Kinv[7] = (K[1] * K[6] - K[0] * K[7]) * id;
    Kinv[8] = (K[0] * K[4] - K[1] * K[3]) * id;
    double X[4][3], uv[4][2];
    for (int k = 0; k < 4; ++k) {
      const float* c = corr + ((size_t)b * HW + s[k]) * 5;  // s[k] < cnt ≤ HW
      X[k][0] = c[0];
      X[k][1] = c[1];
      X[k][2] = c[2];
      uv[k][0] = c[3];
      uv[k][1] = c[4];
    }
    ok = finite_d(id) && p3p_best(X, uv, K, Kinv, R, t);
  }
  float* P = hyp + (size_t)i * 12;
  float* Rt = hyp_rt + (size_t)i * 12;
  if (ok) {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c)
        P[r * 4 + c] = (float)(K[r * 3] * R[c] + K[r * 3 + 1] * R[3 + c] + K[r * 3 + 2] * R[6 + c]);
      P[r * 4 + 3] = (float)(K[r * 3] * t[0] + K[r * 3 + 1] * t[1] + K[r * 3 + 2] * t[2]);
    }
    for (int k = 0; k < 12; ++k) ok = ok && fabsf(P[k]) <= 3.402823466e38f;
  }
  if (!ok) {  // behind the camera for every point: scores 0 even if the flag were ignored
    for (int k = 0; k < 12; ++k) P[k] = k == 11 ? -1.f : 0.f;
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    t[0] = t[1] = t[2] = 0.0;
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rt[r * 4 + c] = (float)R[r * 3 + c];
    Rt[r * 4 + 3] = (float)t[r];
  }
  hyp_valid[i] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------- scoring
// inlier test without a division: z > 0 and |(x, y) − z·(u, v)|² < thr²·z²
__device__ __forceinline__ bool pnp_inlier(const float* __restrict__ P, float X, float Y, float Z,
                                           float u, float v, float thr2) {
  const float x = P[0] * X + P[1] * Y + P[2] * Z + P[3];
  const float y = P[4] * X + P[5] * Y + P[6] * Z + P[7];
  const float z = P[8] * X + P[9] * Y + P[10] * Z + P[11];
  const float ex = x - u * z, ey = y - v * z;
  return z > 0.f && ex * ex + ey * ey < thr2 * (z * z);
}

__global__ __launch_bounds__(256) void score_kernel(const float* __restrict__ corr,
                                                    const int* __restrict__ count,
                                                    const float* __restrict__ hyp,
                                                    const int* __restrict__ hyp_valid,
                                                    int* __restrict__ score, int HW, int hyps,
                                                    float thr2) {
  __shared__ float sP[SCFLOW_PNP_MAX_HYPS * 12];
  __shared__ int sC[SCFLOW_PNP_MAX_HYPS];
  const int b = blockIdx.y;
  const int cnt = min(count[b], HW);
  const int start = blockIdx.x * kChunk;
  if (start >= cnt) return;  // the whole workgroup
  for (int i = threadIdx.x; i < hyps * 12; i += 256) {
    float v = hyp[(size_t)b * hyps * 12 + i];
    if (!hyp_valid[b * hyps + i / 12]) v = (i % 12 == 11) ? -1.f : 0.f;
    sP[i] = v;
  }
  for (int i = threadIdx.x; i < hyps; i += 256) sC[i] = 0;
  float X[4], Y[4], Z[4], u[4], v[4];
  bool act[4];
  for (int j = 0; j < 4; ++j) {
    const int p = start + j * 256 + threadIdx.x;
    act[j] = p < cnt;
    const float* c = corr + ((size_t)b * HW + (act[j] ? p : start)) * 5;
    X[j] = c[0];
    Y[j] = c[1];
    Z[j] = c[2];
    u[j] = c[3];
    v[j] = c[4];
  }
  __syncthreads();
  const bool lane0 = (threadIdx.x & 63) == 0;
  for (int h = 0; h < hyps; ++h) {
    const float* P = sP + h * 12;  // one address for the wave: an LDS broadcast
    int c = 0;
    for (int j = 0; j < 4; ++j)
      c += __popcll(__ballot(act[j] && pnp_inlier(P, X[j], Y[j], Z[j], u[j], v[j], thr2)));
    if (lane0 && c) atomicAdd(&sC[h], c);
  }
  __syncthreads();
  for (int h = threadIdx.x; h < hyps; h += 256)
    if (sC[h]) atomicAdd(&score[b * hyps + h], sC[h]);
}

// ------------------------------------------------------------------------------- refinement
// lower Cholesky of the 6×6 A (in place), then solves A x = g; false on a bad pivot
__device__ bool chol_solve6(double (*A)[6], double* g) {
  for (int i = 0; i < 6; ++i) {
    for (int jx = 0; jx <= i; ++jx) {
      double s = A[i][jx];
      for (int k = 0; k < jx; ++k) s -= A[i][k] * A[jx][k];
      if (i == jx) {
        if (!(s > 0.0) || !finite_d(s)) return false;
        A[i][i] = sqrt(s);
      } else {
        A[i][jx] = s / A[jx][jx];
      }
    }
  }
  for (int i = 0; i < 6; ++i) {
    double s = g[i];
    for (int k = 0; k < i; ++k) s -= A[i][k] * g[k];
    g[i] = s / A[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = g[i];
    for (int k = i + 1; k < 6; ++k) s -= A[k][i] * g[k];
    g[i] = s / A[i][i];
  }
  for (int i = 0; i < 6; ++i)
    if (!finite_d(g[i])) return false;
  return true;
}

constexpr int kRefineThreads = 512;  // 8 waves: 256 VGPRs each hold the 27 fp64 sums unspilled

__global__ __launch_bounds__(kRefineThreads) void refine_kernel(
    const float* __restrict__ corr, const int* __restrict__ count, const float* __restrict__ hyp,
    const float* __restrict__ hyp_rt, const int* __restrict__ hyp_valid,
    const int* __restrict__ score, const float* __restrict__ Kf, const float* __restrict__ Rref,
    const float* __restrict__ tref, float* __restrict__ Rout, float* __restrict__ tout,
    int* __restrict__ okout, int* __restrict__ inl_out, double* __restrict__ pose64, int HW, int hyps,
    float thr2, int iters) {
  __shared__ int s_ok, s_score, s_stop;
  __shared__ float sP[12];
  __shared__ double sK[5];
  __shared__ double sR[9], sT[3];
  __shared__ double sAcc[kRefineThreads / 64][27];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cnt = min(count[b], HW);
  if (tid == 0) {
    int best = 0, bs = -1;
    for (int h = 0; h < hyps; ++h) {
      const int s = score[b * hyps + h];
      if (s > bs) {
        bs = s;
        best = h;
      }
    }
    s_ok = cnt >= 4 && hyp_valid[b * hyps + best] != 0 && bs >= 4;
    s_score = bs;
    s_stop = 0;
    const size_t o = ((size_t)b * hyps + best) * 12;
    for (int k = 0; k < 12; ++k) sP[k] = hyp[o + k];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) sR[r * 3 + c] = (double)hyp_rt[o + r * 4 + c];
      sT[r] = (double)hyp_rt[o + r * 4 + 3];
    }
    // The fp32 start is orthonormal to 3e-8 only, and R ← exp(ω)·R would carry that defect to the
    // end: Gram-Schmidt on the rows in fp64 first.
    {
      double* r0 = sR, *r1 = sR + 3, *r2 = sR + 6;
      const double n0 = 1.0 / sqrt(dot3(r0, r0));
      for (int k = 0; k < 3; ++k) r0[k] *= n0;
      const double d01 = dot3(r0, r1);
      for (int k = 0; k < 3; ++k) r1[k] -= d01 * r0[k];
      const double n1 = 1.0 / sqrt(dot3(r1, r1));
      for (int k = 0; k < 3; ++k) r1[k] *= n1;
      cross3(r0, r1, r2);
    }
    sK[0] = Kf[b * 9 + 0];
    sK[1] = Kf[b * 9 + 1];
    sK[2] = Kf[b * 9 + 2];
    sK[3] = Kf[b * 9 + 4];
    sK[4] = Kf[b * 9 + 5];
  }
  __syncthreads();
  const bool ok = s_ok != 0;
  for (int it = 0; ok && it < iters; ++it) {
    // Residuals and Jacobians in fp64 as well: the fp64 VALU rate of gfx950 equals the fp32 rate,
    // and an fp32 evaluation of R·X + t cannot see a pose change below one fp32 ulp of t_z (6e-5 mm
    // at 1 m), so the iteration would wander at that level instead of converging.
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = sR[k];
    for (int k = 0; k < 3; ++k) t[k] = sT[k];
    const double k00 = sK[0], k01 = sK[1], k02 = sK[2], k11 = sK[3], k12 = sK[4];
    double acc[27];
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (int p = tid; p < cnt; p += kRefineThreads) {
      const float* c = corr + ((size_t)b * HW + p) * 5;
      const float Xf = c[0], Yf = c[1], Zf = c[2], uo = c[3], vo = c[4];
      if (!pnp_inlier(sP, Xf, Yf, Zf, uo, vo, thr2)) continue;
      const double X = Xf, Y = Yf, Z = Zf;
      const double x = R[0] * X + R[1] * Y + R[2] * Z + t[0];
      const double y = R[3] * X + R[4] * Y + R[5] * Z + t[1];
      const double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
      const double iz = 1.0 / z;
      const double su = k00 * x + k01 * y, sv = k11 * y;
      const double ru = (double)uo - (su * iz + k02), rv = (double)vo - (sv * iz + k12);
      const double a0 = k00 * iz, a1 = k01 * iz, a2 = -su * iz * iz;
      const double b1 = k11 * iz, b2 = -sv * iz * iz;
      const double du[6] = {a2 * y - a1 * z, a0 * z - a2 * x, a1 * x - a0 * y, a0, a1, a2};
      const double dv[6] = {b2 * y - b1 * z, -(b2 * x), b1 * x, 0.0, b1, b2};
      int o = 0;
      for (int i = 0; i < 6; ++i)
        for (int jx = 0; jx <= i; ++jx) acc[o++] += du[i] * du[jx] + dv[i] * dv[jx];
      for (int i = 0; i < 6; ++i) acc[21 + i] += du[i] * ru + dv[i] * rv;
    }
    // fixed order: lanes by halving strides, then the waves in turn
    for (int k = 0; k < 27; ++k) {
      double v = acc[k];
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
      if ((tid & 63) == 0) sAcc[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double A[6][6], g[6];
      int o = 0;
      for (int i = 0; i < 6; ++i)
        for (int jx = 0; jx <= i; ++jx, ++o) {
          double s = 0.0;
          for (int w = 0; w < kRefineThreads / 64; ++w) s += sAcc[w][o];
          A[i][jx] = s;
        }
      for (int i = 0; i < 6; ++i) {
        double s = 0.0;
        for (int w = 0; w < kRefineThreads / 64; ++w) s += sAcc[w][21 + i];
        g[i] = s;
      }
      if (!chol_solve6(A, g)) {
        s_stop = 1;  // keep the last pose
      } else {
        const double wx = g[0], wy = g[1], wz = g[2];
        const double th = sqrt(wx * wx + wy * wy + wz * wz);
        double ka = 1.0, kb = 0.0;
        if (th >= 1e-12) {
          ka = sin(th) / th;
          kb = (1.0 - cos(th)) / (th * th);
        }
        const double Wm[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
        double E[9], Rn[9], tn[3];
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) {
            double w2 = 0.0;
            for (int k = 0; k < 3; ++k) w2 += Wm[r * 3 + k] * Wm[k * 3 + c];
            E[r * 3 + c] = (r == c ? 1.0 : 0.0) + ka * Wm[r * 3 + c] + kb * w2;
          }
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c)
            Rn[r * 3 + c] = E[r * 3] * sR[c] + E[r * 3 + 1] * sR[3 + c] + E[r * 3 + 2] * sR[6 + c];
          tn[r] = E[r * 3] * sT[0] + E[r * 3 + 1] * sT[1] + E[r * 3 + 2] * sT[2] + g[3 + r];
        }
        for (int k = 0; k < 9; ++k) sR[k] = Rn[k];
        for (int k = 0; k < 3; ++k) sT[k] = tn[k];
      }
    }
    __syncthreads();
    if (s_stop) break;
  }
  if (tid == 0) {
    bool fin = ok;
    float Ro[9], to[3];
    for (int k = 0; k < 9; ++k) {
      Ro[k] = (float)sR[k];
      fin = fin && fabsf(Ro[k]) <= 3.402823466e38f;
    }
    for (int k = 0; k < 3; ++k) {
      to[k] = (float)sT[k];
      fin = fin && fabsf(to[k]) <= 3.402823466e38f;
    }
    for (int k = 0; k < 9; ++k) Rout[b * 9 + k] = fin ? Ro[k] : Rref[b * 9 + k];
    for (int k = 0; k < 3; ++k) tout[b * 3 + k] = fin ? to[k] : tref[b * 3 + k];
    if (pose64) {  // the unrounded result (R row-major, then t)
      for (int k = 0; k < 9; ++k) pose64[b * 12 + k] = fin ? sR[k] : (double)Rref[b * 9 + k];
      for (int k = 0; k < 3; ++k) pose64[b * 12 + 9 + k] = fin ? sT[k] : (double)tref[b * 3 + k];
    }
    okout[b] = fin ? 1 : 0;
    inl_out[b] = fin ? s_score : 0;
  }
}

long long ws_bytes_for(int n, int h, int w) {
  const long long chunks = ((long long)h * w + kChunk - 1) / kChunk;
  return ((long long)n * chunks * 4 + 15) / 16 * 16;
}

}  // namespace

SCFLOW_API int scflow_pnp_workspace(int n, int h, int w, int hyps, long long* bytes) {
  if (!bytes || n <= 0 || h <= 0 || w <= 0 || hyps <= 0) return SCFLOW_EINVAL;
  if (hyps > SCFLOW_PNP_MAX_HYPS || (long long)h * w > (1 << 24) || (long long)n * h * w >= (1LL << 31))
    return SCFLOW_EUNSUPPORTED;
  *bytes = ws_bytes_for(n, h, w);
  return SCFLOW_OK;
}

SCFLOW_API int scflow_pnp_compact(const float* points, const float* flow, const float* valid,
                                  float* corr, int* count, void* workspace,
                                  long long workspace_bytes, int n, int h, int w, void* stream) {
  if (!points || !flow || !corr || !count || !workspace || n <= 0 || h <= 0 || w <= 0)
    return SCFLOW_EINVAL;
  if ((long long)h * w > (1 << 24) || (long long)n * h * w >= (1LL << 31)) return SCFLOW_EUNSUPPORTED;
  if (workspace_bytes < ws_bytes_for(n, h, w)) return SCFLOW_EINVAL;
  if (!aligned16(points)) return SCFLOW_EALIGN;
  const int HW = h * w;
  const dim3 grid(ceil_div(HW, kChunk), n);
  compact_count_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const floatx4*)points, valid,
                                                              (int*)workspace, HW);
  compact_write_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(
      (const floatx4*)points, flow, valid, (const int*)workspace, corr, count, HW, w);
  return scflow_launch_status();
}

SCFLOW_API int scflow_pnp_hypotheses(const float* corr, const int* count, const float* K,
                                     float* hyp, float* hyp_pose, int* hyp_valid, int* samples,
                                     int n, int hw, int hyps, unsigned seed, void* stream) {
  if (!corr || !count || !K || !hyp || !hyp_pose || !hyp_valid || n <= 0 || hw <= 0 || hyps <= 0)
    return SCFLOW_EINVAL;
  if (hyps > SCFLOW_PNP_MAX_HYPS || (long long)n * hw >= (1LL << 31)) return SCFLOW_EUNSUPPORTED;
  hypotheses_kernel<<<ceil_div((long long)n * hyps, 64), 64, 0, (hipStream_t)stream>>>(
      corr, count, K, hyp, hyp_pose, hyp_valid, samples, n, hw, hyps, (uint32_t)seed);
  return scflow_launch_status();
}

SCFLOW_API int scflow_pnp_score(const float* corr, const int* count, const float* hyp,
                                const int* hyp_valid, int* score, int n, int hw, int hyps,
                                float thr, void* stream) {
  if (!corr || !count || !hyp || !hyp_valid || !score || n <= 0 || hw <= 0 || hyps <= 0 ||
      !(thr > 0.f))
    return SCFLOW_EINVAL;
  if (hyps > SCFLOW_PNP_MAX_HYPS || (long long)n * hw >= (1LL << 31)) return SCFLOW_EUNSUPPORTED;
  const hipError_t e = hipMemsetAsync(score, 0, (size_t)n * hyps * sizeof(int), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  score_kernel<<<dim3(ceil_div(hw, kChunk), n), 256, 0, (hipStream_t)stream>>>(
      corr, count, hyp, hyp_valid, score, hw, hyps, thr * thr);
  return scflow_launch_status();
}

SCFLOW_API int scflow_pnp_refine(const float* corr, const int* count, const float* hyp,
                                 const float* hyp_pose, const int* hyp_valid, const int* score,
                                 const float* K, const float* R_ref, const float* t_ref,
                                 float* R_out, float* t_out, int* ok, int* inliers, double* pose64,
                                 int n, int hw, int hyps, float thr, int refine_iters,
                                 void* stream) {
  if (!corr || !count || !hyp || !hyp_pose || !hyp_valid || !score || !K || !R_ref || !t_ref ||
      !R_out || !t_out || !ok || !inliers || n <= 0 || hw <= 0 || hyps <= 0 || !(thr > 0.f) ||
      refine_iters < 0)
    return SCFLOW_EINVAL;
  if (hyps > SCFLOW_PNP_MAX_HYPS || (long long)n * hw >= (1LL << 31)) return SCFLOW_EUNSUPPORTED;
  refine_kernel<<<n, kRefineThreads, 0, (hipStream_t)stream>>>(
      corr, count, hyp, hyp_pose, hyp_valid, score, K, R_ref, t_ref, R_out, t_out, ok, inliers,
      pose64, hw, hyps, thr * thr, refine_iters);
  return scflow_launch_status();
}
