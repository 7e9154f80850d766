// Training patches from full frames: the reference's training formatting
// PoseJitter → ComputeBbox → Crop(size_range) → RandomHSV → RandomNoise → RandomSmooth → Resize →
// Pad → RemapPose → Normalize (configs/refine_models/scflow_ycbv_real.py:50-93,
// datasets/pipelines/jitter.py:51-79, color_transform.py:78-134) with every random number taken
// from a counter-based generator, so that the host never learns a crop's size or a draw's outcome.
//
//   train_draw_kernel         one workgroup per object: every thread derives the same jitter
//                             candidates from the counter (nothing is broadcast), all threads sum
//                             the ADD of a candidate (wave reduction, then LDS); thread 0 stores.
//   patch_extract_aug_kernel  scflow_patch_extract for uint8 × 3 frames with HSV, noise and box
//                             blur applied to the crop before the resize.  A workgroup owns a tile
//                             of output pixels; it augments the crop window that tile reads (plus
//                             the blur's halo) once into LDS as uint8 × 3 and takes every tap's
//                             window from there.  Where that window exceeds the LDS budget, and for objects
//                             whose stage mask is 0, each tap computes its own window from the
//                             frame (the direct route).  Both routes sum the same integers.
//                             The <true> instantiation (scflow_train_patch_extract_bg, DESIGN.md
//                             §18) draws a background slot per object and replaces every crop
//                             pixel that the instance mask calls background, before the stages;
//                             <false> is the kernel without any of that.
//
// Every fp32 expression here is part of the contract (tests/train_patch_restatement.py restates it
// operation by operation), so contraction into FMAs is off for the whole file.
#include "patch_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int TD_THREADS = 256;
constexpr int PA_LDS_BYTES = 48 * 1024;  // augmented window of one workgroup (two fit in a CU)

// ---------------------------------------------------------------------------------- generator
// Philox4x32-10 (Salmon et al., SC'11), stateless: counter (index, object, stream, step) under the
// 64-bit seed as key.  stream: who consumes the words (SCFLOW_RNG_*); the upper 32 bits of step
// travel in the stream word above its low byte.
struct Words {
  uint32_t w[4];
};

__host__ __device__ inline Words philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                        uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return Words{{c0, c1, c2, c3}};
}

struct Rng {
  unsigned long long seed, step;
  __device__ Words draw(uint32_t index, uint32_t object, uint32_t stream) const {
    return philox(index, object, stream | ((uint32_t)(step >> 32) << 8), (uint32_t)step,
                  (uint32_t)seed, (uint32_t)(seed >> 32));
  }
};

// [0, 1): 24 bits, exact
__device__ inline float u01(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }
// (0, 1]: the sum has 25 bits and is rounded to 24, so the largest word gives 1 (and a normal of 0)
__device__ inline float u01_open(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 0x1p-24f; }

// three normals of one Philox call by Box–Muller: (w0, w1) → z0 (cos), z1 (sin); (w2, w3) → z2
__device__ __forceinline__ void normal3(const Words& q, float* z) {
  const float r0 = sqrtf(-2.f * logf(u01_open(q.w[0]))), a0 = 6.2831853071795865f * u01(q.w[1]);
  const float r1 = sqrtf(-2.f * logf(u01_open(q.w[2]))), a1 = 6.2831853071795865f * u01(q.w[3]);
  z[0] = r0 * cosf(a0), z[1] = r0 * sinf(a0), z[2] = r1 * cosf(a1);
}

// ---------------------------------------------------------------------------------- draw
struct TrainDrawArgs {
  const float* points;
  const int* counts;
  const int* labels;
  const float* diameters;
  const float* R_gt;
  const float* t_gt;
  float* R_ref;
  float* t_ref;
  float* errors;
  unsigned char* ok;
  int* tries;
  float* ratio;
  float* aug;
  float cfg[SCFLOW_TRAIN_CFG_LEN];
  int num_classes, max_points, max_tries, num_kernels;
  uint32_t object_offset;
  Rng rng;
};

__global__ __launch_bounds__(TD_THREADS) void train_draw_kernel(TrainDrawArgs a) {
  __shared__ float red[2][TD_THREADS / 64];  // double-buffered: one barrier per try
  const int i = blockIdx.x, tid = threadIdx.x;
  const uint32_t obj = (uint32_t)i + a.object_offset;
  const float* cfg = a.cfg;
  const int label = a.labels[i];
  int cnt = 0;
  float diam = 0.f;
  if (label >= 0 && label < a.num_classes) {
    cnt = a.counts[label];
    cnt = cnt < 0 ? 0 : (cnt > a.max_points ? a.max_points : cnt);
    diam = a.diameters[label];
  }
  const float* pts = a.points + (size_t)(cnt ? label : 0) * a.max_points * 3;
  float Rg[9], tg[3];
  for (int j = 0; j < 9; ++j) Rg[j] = a.R_gt[9 * (size_t)i + j];
  for (int j = 0; j < 3; ++j) tg[j] = a.t_gt[3 * (size_t)i + j];
  const float ang_lim = cfg[SCFLOW_TRAIN_ANGLE_LIMIT], tr_lim = cfg[SCFLOW_TRAIN_TRANS_LIMIT];
  const float add_lim = cfg[SCFLOW_TRAIN_ADD_LIMIT];
  const bool use_add = add_lim >= 0.f && cnt > 0 && diam > 0.f;

  float Rr[9], tr[3], e_add = 0.f, e_rot = 0.f, e_tr = 0.f;
  int ok = 0, tries = a.max_tries, buf = 0;
  for (int k = 0; k < a.max_tries; ++k) {  // every thread takes the same path through this loop
    float z[3], dt[3];
    normal3(a.rng.draw(0, obj, SCFLOW_RNG_JITTER + k), z);
    float cs[3], sn[3];
    for (int j = 0; j < 3; ++j) {
      const float deg = cfg[SCFLOW_TRAIN_ANGLE_MEAN] + cfg[SCFLOW_TRAIN_ANGLE_STD] * z[j];
      const float rad = deg * 0.017453292519943295f;
      cs[j] = cosf(rad), sn[j] = sinf(rad);
    }
    // ΔR = Rx(c)·Ry(b)·Rz(a): scipy's from_euler('zyx', (a, b, c))
    const float Rz[9] = {cs[0], -sn[0], 0.f, sn[0], cs[0], 0.f, 0.f, 0.f, 1.f};
    const float Ry[9] = {cs[1], 0.f, sn[1], 0.f, 1.f, 0.f, -sn[1], 0.f, cs[1]};
    const float Rx[9] = {1.f, 0.f, 0.f, 0.f, cs[2], -sn[2], 0.f, sn[2], cs[2]};
    float yz[9], dR[9], cand[9];
    mat3_mul(Ry, Rz, yz);
    mat3_mul(Rx, yz, dR);
    mat3_mul(dR, Rg, cand);
    float trace = 0.f;  // tr(R_ref·R_gtᵀ)
    for (int j = 0; j < 9; ++j) trace = trace + cand[j] * Rg[j];
    const float cosang = fminf(fmaxf((trace - 1.f) / 2.f, -1.f), 1.f);
    const float rot = acosf(cosang) * 57.29577951308232f;
    if (ang_lim >= 0.f && rot > ang_lim) continue;

    normal3(a.rng.draw(1, obj, SCFLOW_RNG_JITTER + k), z);
    for (int j = 0; j < 3; ++j)
      dt[j] = cfg[SCFLOW_TRAIN_T_MEAN + j] + cfg[SCFLOW_TRAIN_T_STD + j] * z[j];
    const float tn = sqrtf((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]);
    if (tr_lim >= 0.f && tn > tr_lim) continue;

    float add = 0.f;
    if (cnt > 0 && diam > 0.f) {
      float part = 0.f;
      for (int p = tid; p < cnt; p += TD_THREADS) {
        const float X = pts[3 * p], Y = pts[3 * p + 1], Z = pts[3 * p + 2];
        float d2 = 0.f;
        for (int r = 0; r < 3; ++r) {
          const float g = ((Rg[3 * r] * X + Rg[3 * r + 1] * Y) + Rg[3 * r + 2] * Z) + tg[r];
          const float c = ((cand[3 * r] * X + cand[3 * r + 1] * Y) + cand[3 * r + 2] * Z) +
                          (tg[r] + dt[r]);
          d2 = d2 + (g - c) * (g - c);
        }
        part = part + sqrtf(d2);
      }
      for (int off = 32; off; off >>= 1) part = part + __shfl_xor(part, off);
      if ((tid & 63) == 0) red[buf][tid >> 6] = part;
      __syncthreads();
      float sum = red[buf][0];
      for (int w = 1; w < TD_THREADS / 64; ++w) sum = sum + red[buf][w];
      buf ^= 1;  // the next try writes the other buffer, so no second barrier is needed
      add = (sum / (float)cnt) / diam;
    }
    if (use_add && add > add_lim) continue;
    for (int j = 0; j < 9; ++j) Rr[j] = cand[j];
    for (int j = 0; j < 3; ++j) tr[j] = tg[j] + dt[j];
    e_add = add, e_rot = rot, e_tr = tn, ok = 1, tries = k + 1;
    break;
  }
  if (tid != 0) return;
  if (!ok) {
    for (int j = 0; j < 9; ++j) Rr[j] = Rg[j];
    for (int j = 0; j < 3; ++j) tr[j] = tg[j];
  }
  for (int j = 0; j < 9; ++j) a.R_ref[9 * (size_t)i + j] = Rr[j];
  for (int j = 0; j < 3; ++j) a.t_ref[3 * (size_t)i + j] = tr[j];
  a.errors[3 * (size_t)i] = e_add, a.errors[3 * (size_t)i + 1] = e_rot;
  a.errors[3 * (size_t)i + 2] = e_tr;
  a.ok[i] = (unsigned char)ok, a.tries[i] = tries;

  const Words qr = a.rng.draw(0, obj, SCFLOW_RNG_CROP);
  const float lo = cfg[SCFLOW_TRAIN_RATIO_LO], hi = cfg[SCFLOW_TRAIN_RATIO_HI];
  a.ratio[i] = lo + u01(qr.w[0]) * (hi - lo);
  const Words q0 = a.rng.draw(0, obj, SCFLOW_RNG_COLOUR), q1 = a.rng.draw(1, obj, SCFLOW_RNG_COLOUR);
  float* row = a.aug + 8 * (size_t)i;
  for (int j = 0; j < 3; ++j)
    row[j] = 1.f + (2.f * u01(q0.w[j]) - 1.f) * cfg[SCFLOW_TRAIN_H_RATIO + j];
  row[3] = u01(q0.w[3]) * cfg[SCFLOW_TRAIN_NOISE_RATIO];
  int ki = (int)(u01(q1.w[0]) * (float)a.num_kernels);
  ki = ki < a.num_kernels - 1 ? ki : a.num_kernels - 1;
  row[4] = (float)(2 * ki + 1);
  int mask = 0;
  for (int j = 0; j < 3; ++j) mask |= (u01(q1.w[1 + j]) <= cfg[SCFLOW_TRAIN_P_HSV + j]) << j;
  row[5] = (float)mask, row[6] = 0.f, row[7] = 0.f;
}

// ---------------------------------------------------------------------------------- stages
struct Px {
  int b, g, r;
};

// cv2's 8-bit BGR → HSV (H in [0, 180)) in integers, the gains in fp32, and its 8-bit HSV → BGR
__device__ __forceinline__ Px hsv_stage(Px p, float ga, float gb, float gc) {
  const int v = max(p.b, max(p.g, p.r)), mn = min(p.b, min(p.g, p.r)), d = v - mn;
  const int sdiv = v ? (2 * (255 << 12) + v) / (2 * v) : 0;        // round((255 << 12) / v)
  const int hdiv = d ? (2 * ((180 << 12) / 6) + d) / (2 * d) : 0;  // round((180 << 12) / (6·d))
  const int s = (d * sdiv + 2048) >> 12;
  const int h0 = v == p.r ? p.g - p.b : (v == p.g ? p.b - p.r + 2 * d : p.r - p.g + 4 * d);
  int h = (h0 * hdiv + 2048) >> 12;  // arithmetic shift: floor, as cv2's
  h += h < 0 ? 180 : 0;
  float hf = (float)h * ga, sf = (float)s * gb, vf = (float)v * gc;
  if (ga >= 1.f) hf = fminf(hf, 179.f);
  if (gb >= 1.f) sf = fminf(sf, 255.f);
  if (gc >= 1.f) vf = fminf(vf, 255.f);
  // truncation to uint8; a gain below 1 cannot exceed the range, a negative one is held at 0
  const int hq = (int)fminf(fmaxf(hf, 0.f), 179.f), sq = (int)fminf(fmaxf(sf, 0.f), 255.f);
  const int vq = (int)fminf(fmaxf(vf, 0.f), 255.f);
  float out[3];
  const float vv = (float)vq * (1.f / 255.f);
  if (sq == 0) {
    out[0] = out[1] = out[2] = vv;
  } else {
    const float hh = (float)hq * (6.f / 180.f), ss = (float)sq * (1.f / 255.f);
    const float fl = floorf(hh), f = hh - fl;
    int sector = (int)fl;
    sector = sector > 5 ? 5 : sector;
    const float tab[4] = {vv, vv * (1.f - ss), vv * (1.f - ss * f), vv * (1.f - ss * (1.f - f))};
    const int sel[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};
    // selects, not a runtime-indexed array: keeps tab in registers
    for (int c = 0; c < 3; ++c) {
      const int t = sel[sector][c];
      out[c] = t == 0 ? tab[0] : (t == 1 ? tab[1] : (t == 2 ? tab[2] : tab[3]));
    }
  }
  Px q;
  q.b = (int)fminf(fmaxf(rintf(out[0] * 255.f), 0.f), 255.f);
  q.g = (int)fminf(fmaxf(rintf(out[1] * 255.f), 0.f), 255.f);
  q.r = (int)fminf(fmaxf(rintf(out[2] * 255.f), 0.f), 255.f);
  return q;
}

__device__ inline int noise_level(int x, float z, float sigma) {
  const float y = (float)x + (z * sigma) * 255.f;
  return (int)fminf(fmaxf(y, 0.f), 255.f);
}

// BORDER_REFLECT_101 on an axis of n samples: period 2(n − 1); one sample folds to 0
__device__ inline int fold101(int p, int n) {
  if ((unsigned)p < (unsigned)n) return p;  // inside: no division
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  p %= period;
  p += p < 0 ? period : 0;
  return p > n - 1 ? period - p : p;
}

struct PatchAugArgs {
  const unsigned char* frames;
  const int* frame_index;
  const int* geom;
  const unsigned char* valid;
  const float* aug;
  float* out;
  int F, H, W, S;
  int pad;
  float mean[3], std[3];
  int to_rgb, quantize, direct;
  uint32_t object_offset;
  Rng rng;
};

// RandomBackground (color_transform.py:177-244): what the <true> instantiation takes on top
struct BgArgs {
  const unsigned char* masks;  // [F][H][W], foreground where != 0
  const unsigned char* pool;   // [B][Hb][Wb][3] BGR
  const int* sizes;            // [B][2] used (height, width), top-left aligned; NULL: whole slots
  const int* choice;           // [n] −1 none, 0 .. B−1 that slot; NULL: drawn
  int* chosen;                 // [n] the slot applied, −1 for none
  int B, Hb, Wb;
  float p;
};

// what a workgroup knows of its object
struct Crop {
  const unsigned char* frame;
  int x1, y1, cw, ch, H, W, pad, mask;
  float ga, gb, gc, sigma;
  uint32_t obj;
  // the background's used region and the frame's mask; bg == nullptr: no background
  const unsigned char* bg;
  const unsigned char* fmask;
  int bw, bh, bstride;
};

// linear_coord for a background axis: (2o + 1)·n reaches 2^35 at the accepted limits (a crop side
// of PX_MAX_CROP on a slot side of PX_MAX_ORIGIN), so the wide case divides in 64 bits.  Which
// case runs is the same for a whole object.
__device__ inline void bg_coord(int o, int n, int no, int& i0, float& f) {
  if ((long long)(2 * no) * n < (1ll << 31)) return linear_coord(o, n, no, i0, f);
  const long long num = (long long)(2 * o + 1) * n - no, den = 2 * no;
  if (num < 0) {
    i0 = 0, f = 0.f;
    return;
  }
  const long long q = num / den;
  i0 = (int)q;
  f = (float)(num - q * den) / (float)den;
  if (i0 >= n - 1) i0 = n - 1, f = 0.f;
}

// crop pixel (x, y) of the background resized to the crop's cw × ch: the resample of DESIGN.md §15
// (cv2's INTER_LINEAR, aspect ratio not kept) on the used region, rounded to a level
__device__ __forceinline__ Px bg_pixel(const Crop& c, int x, int y) {
  int xa, ya;
  float fx, fy;
  bg_coord(x, c.bw, c.cw, xa, fx);
  bg_coord(y, c.bh, c.ch, ya, fy);
  const int xb = xa + 1 < c.bw - 1 ? xa + 1 : c.bw - 1, yb = ya + 1 < c.bh - 1 ? ya + 1 : c.bh - 1;
  const unsigned char* r0 = c.bg + (size_t)ya * c.bstride;
  const unsigned char* r1 = c.bg + (size_t)yb * c.bstride;
  const float gx = 1.f - fx, gy = 1.f - fy;
  int v[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float up = gx * (float)r0[3 * xa + ch] + fx * (float)r0[3 * xb + ch];
    const float dn = gx * (float)r1[3 * xa + ch] + fx * (float)r1[3 * xb + ch];
    v[ch] = (int)rintf(gy * up + fy * dn);
  }
  return Px{v[0], v[1], v[2]};
}

// crop pixel (x, y), 0 ≤ x < cw, 0 ≤ y < ch, after HSV and noise.  BG: under a background, a
// pixel outside the frame or with a zero mask byte is the background's instead (a select)
template <bool BG>
__device__ __forceinline__ Px aug_pixel(const Crop& c, const Rng& rng, int x, int y) {
  const int fx = c.x1 + x, fy = c.y1 + y;
  Px p{c.pad, c.pad, c.pad};
  bool in = fx >= 0 && fx < c.W && fy >= 0 && fy < c.H;
  if constexpr (BG) {
    if (c.bg) {
      in = in && c.fmask[(size_t)fy * c.W + fx] != 0;
      if (!in) p = bg_pixel(c, x, y);
    }
  }
  if (in) {
    const unsigned char* s = c.frame + ((size_t)fy * c.W + fx) * 3;
    p.b = s[0], p.g = s[1], p.r = s[2];
  }
  if (c.mask & SCFLOW_AUG_HSV) p = hsv_stage(p, c.ga, c.gb, c.gc);
  if (c.mask & SCFLOW_AUG_NOISE) {
    float z[3];
    normal3(rng.draw((uint32_t)(y * c.cw + x), c.obj, SCFLOW_RNG_NOISE), z);
    p.b = noise_level(p.b, z[0], c.sigma), p.g = noise_level(p.g, z[1], c.sigma);
    p.r = noise_level(p.r, z[2], c.sigma);
  }
  return p;
}

// the k × k box blur of crop pixel (x, y) from a pixel source src(xu, yu) that takes unfolded
// coordinates: level = (2·Σ + k²) div (2·k²)
template <class Src>
__device__ __forceinline__ Px blur_tap(const Src& src, int x, int y, int k) {
  if (k == 1) return src(x, y);
  const int h = k >> 1;
  int sb = 0, sg = 0, sr = 0;
  for (int dy = -h; dy <= h; ++dy)
    for (int dx = -h; dx <= h; ++dx) {
      const Px p = src(x + dx, y + dy);
      sb += p.b, sg += p.g, sr += p.r;
    }
  if (k == 3)  // constant divisors: a multiplication and a shift each
    return Px{(2 * sb + 9) / 18, (2 * sg + 9) / 18, (2 * sr + 9) / 18};
  return Px{(2 * sb + 25) / 50, (2 * sg + 25) / 50, (2 * sr + 25) / 50};
}

// the output tile of a workgroup: 64 columns (the patch's width below that) of 1024 output pixels,
// four neighbouring ones per thread.  16 × 64 keeps the share of halo pixels a blur adds to the
// window low and gives 32 objects at 256² enough workgroups (2048) to fill the device
__host__ __device__ inline int pa_cols(int S) { return S < 64 ? S : 64; }
__host__ __device__ inline int pa_rows(int S) {
  const int r = 1024 / pa_cols(S);
  return r > S ? S : r;
}

template <bool BG>
__global__ __launch_bounds__(PX_THREADS) void patch_extract_aug_kernel(PatchAugArgs a, BgArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char win[];  // PA_LDS_BYTES
  const int S = a.S, rows = pa_rows(S), cols = pa_cols(S);
  const int bands = (S + rows - 1) / rows, ctiles = (S + cols - 1) / cols;
  const int obj = blockIdx.x / (bands * ctiles), tile = blockIdx.x % (bands * ctiles);
  const int row0 = (tile / ctiles) * rows, col0 = (tile % ctiles) * cols, tid = threadIdx.x;
  const int nrows = row0 + rows <= S ? rows : S - row0;
  const int ncols = col0 + cols <= S ? cols : S - col0;

  const int* gp = a.geom + 8 * (size_t)obj;
  const int x1 = gp[0], y1 = gp[1], x2 = gp[2], y2 = gp[3];
  const int nw = gp[4], nh = gp[5], left = gp[6], top = gp[7];
  const int fi = a.frame_index[obj];
  // as in patch_extract_kernel: anything that is not a patch geometry is an invalid object
  const bool ok = a.valid[obj] != 0 && fi >= 0 && fi < a.F && x1 >= -PX_MAX_ORIGIN &&
                  x1 <= PX_MAX_ORIGIN && y1 >= -PX_MAX_ORIGIN && y1 <= PX_MAX_ORIGIN && x2 >= x1 &&
                  y2 >= y1 && x2 - x1 < PX_MAX_CROP && y2 - y1 < PX_MAX_CROP && nw >= 1 &&
                  nh >= 1 && left >= 0 && top >= 0 && nw <= S - left && nh <= S - top;
  Crop c;
  c.cw = ok ? x2 - x1 + 1 : 1, c.ch = ok ? y2 - y1 + 1 : 1;
  c.x1 = x1, c.y1 = y1, c.H = a.H, c.W = a.W, c.pad = a.pad;
  c.frame = a.frames + (size_t)(ok ? fi : 0) * a.H * a.W * 3;
  c.obj = (uint32_t)obj + a.object_offset;
  const float* row = a.aug + 8 * (size_t)obj;
  c.ga = row[0], c.gb = row[1], c.gc = row[2], c.sigma = row[3];
  const float mf = row[5];
  c.mask = mf >= 0.f && mf < 8.f ? (int)mf : 0;  // anything else (a NaN too) switches all stages off
  int k = 1;
  if (c.mask & SCFLOW_AUG_BLUR) k = row[4] == 3.f ? 3 : (row[4] == 5.f ? 5 : 1);
  const int halo = k >> 1;
  c.bg = nullptr;
  if constexpr (BG) {
    // every workgroup of the object derives the same slot from the counter; the first stores it
    int slot = -1;
    if (g.choice) {
      const int v = g.choice[obj];
      slot = v >= 0 && v < g.B ? v : -1;
    } else {
      const Words q = a.rng.draw(0, c.obj, SCFLOW_RNG_BACKGROUND);
      if (u01(q.w[0]) <= g.p) {
        slot = (int)(u01(q.w[1]) * (float)g.B);
        slot = slot < g.B - 1 ? slot : g.B - 1;
      }
    }
    if (slot >= 0) {
      c.bh = g.sizes ? g.sizes[2 * slot] : g.Hb, c.bw = g.sizes ? g.sizes[2 * slot + 1] : g.Wb;
      // a used size that is none refuses the background instead of reading past the slot
      if (c.bh < 1 || c.bh > g.Hb || c.bw < 1 || c.bw > g.Wb) slot = -1;
    }
    if (tile == 0 && tid == 0) g.chosen[obj] = slot;
    if (ok && slot >= 0) {
      c.bstride = 3 * g.Wb;
      c.bg = g.pool + (size_t)slot * g.Hb * c.bstride;
      c.fmask = g.masks + (size_t)fi * a.H * a.W;
    }
  }

  // the tile's rows and columns of the resized crop and the crop window their taps read
  int oya = row0 - top, oyb = row0 + nrows - 1 - top;
  int oxa = col0 - left, oxb = col0 + ncols - 1 - left;
  oya = oya < 0 ? 0 : oya, oyb = oyb > nh - 1 ? nh - 1 : oyb;
  oxa = oxa < 0 ? 0 : oxa, oxb = oxb > nw - 1 ? nw - 1 : oxb;
  const bool any = ok && oya <= oyb && oxa <= oxb;
  int ylo = 0, yhi = 0, xlo = 0, xhi = 0;
  if (any) {
    float f;
    linear_coord(oya, c.ch, nh, ylo, f);
    linear_coord(oyb, c.ch, nh, yhi, f);
    yhi = yhi + 1 < c.ch - 1 ? yhi + 1 : c.ch - 1;
    linear_coord(oxa, c.cw, nw, xlo, f);
    linear_coord(oxb, c.cw, nw, xhi, f);
    xhi = xhi + 1 < c.cw - 1 ? xhi + 1 : c.cw - 1;
  }
  const int wy0 = ylo - halo, wrows = yhi - ylo + 1 + 2 * halo;
  const int wx0 = xlo - halo, wcols = xhi - xlo + 1 + 2 * halo;
  const int wstride = 3 * wcols;
  // block-uniform; a stage mask of 0 leaves nothing to share between taps but the frame itself
  // (under a background: its resampled pixels, so such a window is staged too)
  const bool tiled = any && !a.direct && (c.mask != 0 || (BG && c.bg)) &&
                     (long long)wrows * wstride <= (long long)PA_LDS_BYTES;
  if (tiled) {
    for (int idx = tid; idx < wrows * wcols; idx += PX_THREADS) {
      const int r = idx / wcols, col = idx - r * wcols;
      const Px p = aug_pixel<BG>(c, a.rng, fold101(wx0 + col, c.cw), fold101(wy0 + r, c.ch));
      unsigned char* d = win + r * wstride + 3 * col;
      d[0] = (unsigned char)p.b, d[1] = (unsigned char)p.g, d[2] = (unsigned char)p.r;
    }
    __syncthreads();
  }
  const auto from_lds = [&](int xu, int yu) {
    const unsigned char* s = win + (yu - wy0) * wstride + 3 * (xu - wx0);
    return Px{s[0], s[1], s[2]};
  };
  const auto from_frame = [&](int xu, int yu) {
    return aug_pixel<BG>(c, a.rng, fold101(xu, c.cw), fold101(yu, c.ch));
  };

  const int quads = ncols / 4;
  for (int item = tid; item < nrows * quads; item += PX_THREADS) {
    const int rr = item / quads, q = col0 / 4 + (item - rr * quads);
    const int dy = row0 + rr, oy = dy - top;
    const bool row_in = ok && oy >= 0 && oy < nh;
    int ya = 0, yb = 0;
    float fy = 0.f;
    if (row_in) {
      linear_coord(oy, c.ch, nh, ya, fy);
      yb = ya + 1 < c.ch - 1 ? ya + 1 : c.ch - 1;
    }
    const float gy = 1.f - fy;
    float v[3][4];
    for (int e = 0; e < 4; ++e) {
      const int ox = 4 * q + e - left;
      const bool pin = row_in && ox >= 0 && ox < nw;
      float val[3] = {0.f, 0.f, 0.f};
      if (pin) {
        int xa;
        float fx;
        linear_coord(ox, c.cw, nw, xa, fx);
        const int xb = xa + 1 < c.cw - 1 ? xa + 1 : c.cw - 1;
        Px t[4];
        if (tiled) {
          t[0] = blur_tap(from_lds, xa, ya, k), t[1] = blur_tap(from_lds, xb, ya, k);
          t[2] = blur_tap(from_lds, xa, yb, k), t[3] = blur_tap(from_lds, xb, yb, k);
        } else {
          t[0] = blur_tap(from_frame, xa, ya, k), t[1] = blur_tap(from_frame, xb, ya, k);
          t[2] = blur_tap(from_frame, xa, yb, k), t[3] = blur_tap(from_frame, xb, yb, k);
        }
        const float gx = 1.f - fx;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          float p[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) p[j] = (float)(ch == 0 ? t[j].b : (ch == 1 ? t[j].g : t[j].r));
          const float up = gx * p[0] + fx * p[1], dn = gx * p[2] + fx * p[3];
          float x = gy * up + fy * dn;
          if (a.quantize) x = rintf(x);
          val[ch] = x;
        }
      }
#pragma unroll
      for (int co = 0; co < 3; ++co) {  // selects, not a runtime index: val stays in registers
        const float padn = ((float)a.pad - a.mean[co]) / a.std[co];
        const float x = a.to_rgb ? val[2 - co] : val[co];
        v[co][e] = pin ? (x - a.mean[co]) / a.std[co] : padn;
      }
    }
#pragma unroll
    for (int co = 0; co < 3; ++co) {
      float* o = a.out + (((size_t)obj * 3 + co) * S + dy) * S + 4 * q;
      *(floatx4*)o = floatx4{v[co][0], v[co][1], v[co][2], v[co][3]};
    }
  }
}

}  // namespace

SCFLOW_API void scflow_philox4x32(const unsigned int* counter, const unsigned int* key,
                                  unsigned int* out) {
  if (!counter || !key || !out) return;
  const Words w = philox(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
  for (int j = 0; j < 4; ++j) out[j] = w.w[j];
}

SCFLOW_API int scflow_train_draw(const float* points, const int* counts, const int* labels,
                                 const float* diameters, const float* R_gt, const float* t_gt,
                                 const float* cfg, float* R_ref, float* t_ref, float* errors,
                                 unsigned char* ok, int* tries, float* ratio, float* aug, int n,
                                 int num_classes, int max_points, int max_tries, int max_kernel_size,
                                 unsigned long long seed, unsigned long long step,
                                 unsigned int object_offset, void* stream) {
  if (!points || !counts || !labels || !diameters || !R_gt || !t_gt || !cfg || !R_ref || !t_ref ||
      !errors || !ok || !tries || !ratio || !aug || n <= 0 || num_classes <= 0 || max_points <= 0 ||
      max_tries < 0 || max_kernel_size < 1)
    return SCFLOW_EINVAL;
  if (max_tries > SCFLOW_TRAIN_MAX_TRIES || max_kernel_size > 5 || (step >> 56) ||
      (long long)num_classes * max_points > (1ll << 28))
    return SCFLOW_EUNSUPPORTED;
  TrainDrawArgs a{};
  a.points = points, a.counts = counts, a.labels = labels, a.diameters = diameters;
  a.R_gt = R_gt, a.t_gt = t_gt, a.R_ref = R_ref, a.t_ref = t_ref, a.errors = errors, a.ok = ok;
  a.tries = tries, a.ratio = ratio, a.aug = aug;
  for (int j = 0; j < SCFLOW_TRAIN_CFG_LEN; ++j) a.cfg[j] = cfg[j];
  a.num_classes = num_classes, a.max_points = max_points, a.max_tries = max_tries;
  a.num_kernels = (max_kernel_size + 1) / 2, a.object_offset = object_offset;
  a.rng = Rng{seed, step};
  hipLaunchKernelGGL(train_draw_kernel, dim3(n), dim3(TD_THREADS), 0, (hipStream_t)stream, a);
  return scflow_launch_status();
}

// the checks and the launch both extract entries share; bg == nullptr: the kernel without a background
static int train_extract(const void* frames, const int* frame_index, const int* geom,
                         const unsigned char* valid, const float* aug, float* out, int n,
                         int num_frames, int height, int width, int size, int pad, const float* mean,
                         const float* std, int flags, unsigned long long seed,
                         unsigned long long step, unsigned int object_offset, const BgArgs* bg,
                         void* stream) {
  if (!frames || !frame_index || !geom || !valid || !aug || !out || n <= 0 || num_frames <= 0 ||
      height <= 0 || width <= 0 || pad < 0 || pad > 255 ||
      (flags & ~(SCFLOW_PATCH_TO_RGB | SCFLOW_PATCH_QUANTIZE | SCFLOW_PATCH_AUG_DIRECT)))
    return SCFLOW_EINVAL;
  // !(p >= 0 && p <= 1) refuses a NaN too
  if (bg && (!bg->masks || !bg->pool || !bg->chosen || bg->B <= 0 || bg->Hb <= 0 || bg->Wb <= 0 ||
             !(bg->p >= 0.f && bg->p <= 1.f)))
    return SCFLOW_EINVAL;
  if (size < 4 || size > 4096 || size % 4 || height > PX_MAX_ORIGIN || width > PX_MAX_ORIGIN ||
      (step >> 56))
    return SCFLOW_EUNSUPPORTED;
  if (bg && (bg->Hb > PX_MAX_ORIGIN || bg->Wb > PX_MAX_ORIGIN)) return SCFLOW_EUNSUPPORTED;
  const int rows = pa_rows(size), cols = pa_cols(size);
  const long long tiles = (long long)((size + rows - 1) / rows) * ((size + cols - 1) / cols);
  if (n * tiles >= (1ll << 31)) return SCFLOW_EUNSUPPORTED;
  if (!aligned16(out)) return SCFLOW_EALIGN;
  PatchAugArgs a{};
  a.frames = (const unsigned char*)frames, a.frame_index = frame_index, a.geom = geom;
  a.valid = valid, a.aug = aug, a.out = out;
  a.F = num_frames, a.H = height, a.W = width, a.S = size, a.pad = pad;
  for (int c = 0; c < 3; ++c) a.mean[c] = mean ? mean[c] : 0.f, a.std[c] = std ? std[c] : 1.f;
  a.to_rgb = (flags & SCFLOW_PATCH_TO_RGB) != 0, a.quantize = (flags & SCFLOW_PATCH_QUANTIZE) != 0;
  a.direct = (flags & SCFLOW_PATCH_AUG_DIRECT) != 0;
  a.object_offset = object_offset, a.rng = Rng{seed, step};
  const dim3 grid((unsigned)(n * tiles));
  if (bg)
    hipLaunchKernelGGL(patch_extract_aug_kernel<true>, grid, dim3(PX_THREADS), PA_LDS_BYTES,
                       (hipStream_t)stream, a, *bg);
  else
    hipLaunchKernelGGL(patch_extract_aug_kernel<false>, grid, dim3(PX_THREADS), PA_LDS_BYTES,
                       (hipStream_t)stream, a, BgArgs{});
  return scflow_launch_status();
}

SCFLOW_API int scflow_train_patch_extract(const void* frames, const int* frame_index, const int* geom,
                                        const unsigned char* valid, const float* aug, float* out,
                                        int n, int num_frames, int height, int width, int size,
                                        int pad, const float* mean, const float* std, int flags,
                                        unsigned long long seed, unsigned long long step,
                                        unsigned int object_offset, void* stream) {
  return train_extract(frames, frame_index, geom, valid, aug, out, n, num_frames, height, width,
                       size, pad, mean, std, flags, seed, step, object_offset, nullptr, stream);
}

SCFLOW_API int scflow_train_patch_extract_bg(
    const void* frames, const int* frame_index, const int* geom, const unsigned char* valid,
    const float* aug, float* out, const unsigned char* masks, const unsigned char* pool,
    const int* pool_sizes, const int* choice, int* chosen, int n, int num_frames, int height,
    int width, int size, int pad, const float* mean, const float* std, int flags, int num_slots,
    int pool_height, int pool_width, float p, unsigned long long seed, unsigned long long step,
    unsigned int object_offset, void* stream) {
  const BgArgs bg{masks, pool, pool_sizes, choice, chosen, num_slots, pool_height, pool_width, p};
  return train_extract(frames, frame_index, geom, valid, aug, out, n, num_frames, height, width,
                       size, pad, mean, std, flags, seed, step, object_offset, &bg, stream);
}
