// fp32 MFMA rate vs instruction mix: number of independent accumulators per wave, and
// independent VALU work between the MFMAs — NVALU packed ops (v_pk_fma_f32) per MFMA, or the same
// arithmetic as 2·NVALU scalar ops (FORM 1: v_fma_f32, FORM 2: v_sub_f32), which is what a float2
// operation costs when the compiler splits it.  FORM 0 leaves the float2 expression to the
// compiler, which splits about half of them (tools/isa_loops.py on this file's assembly: 7
// v_pk_fma_f32 + 18 v_fma_f32 where 16 packed ops are written); FORM 3 is the packed op itself.
// usage: ./mfma_mix
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx2 __attribute__((ext_vector_type(2)));

template <int NACC, int NVALU, int FORM = 0>
__global__ __launch_bounds__(256, 2) void mix(float* out, int iters, float a0) {
  floatx16 c[NACC];
  for (int k = 0; k < NACC; ++k) c[k] = floatx16{};
  floatx2 v[8];
  for (int k = 0; k < 8; ++k) v[k] = floatx2{a0 + k, a0 - k};
  const floatx2 m = {1.0001f, 0.9999f};
  float a = a0 + threadIdx.x * 1e-7f, b = 1.0f - threadIdx.x * 1e-7f;
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int r = 0; r < 8 / NACC + (NACC > 8); ++r)
#pragma unroll
      for (int k = 0; k < NACC; ++k) {
        c[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c[k], 0, 0, 0);
#pragma unroll
        for (int q = 0; q < NVALU; ++q) {
          floatx2& d = v[q & 7];
          const floatx2 o = v[(q + 3) & 7];
          if constexpr (FORM == 0) {
            d = d * m + o;
          } else if constexpr (FORM == 3) {
            asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(d) : "v"(m), "v"(o));
          } else {  // one asm per scalar op: the compiler can neither pack nor reorder them away
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              if constexpr (FORM == 1)
                asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(d[h]) : "v"(m[h]), "v"(o[h]));
              else
                asm volatile("v_sub_f32 %0, %0, %1" : "+v"(d[h]) : "v"(o[h]));
            }
          }
        }
      }
  }
  float s = 0.f;
  for (int k = 0; k < NACC; ++k)
    for (int e = 0; e < 16; ++e) s += c[k][e];
  for (int k = 0; k < 8; ++k) s += v[k][0] + v[k][1];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int NACC, int NVALU, int FORM = 0>
void run(float* out, int cus) {
  const int iters = 4000, blocks = cus * 2;
  hipEvent_t s, e;
  (void)hipEventCreate(&s);
  (void)hipEventCreate(&e);
  mix<NACC, NVALU, FORM><<<blocks, 256>>>(out, 10, 1.f);
  (void)hipEventRecord(s);
  mix<NACC, NVALU, FORM><<<blocks, 256>>>(out, iters, 1.f);
  (void)hipEventRecord(e);
  (void)hipEventSynchronize(e);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, s, e);
  const int per_iter = (8 / NACC + (NACC > 8)) * NACC;
  const double flops = (double)blocks * 4 * iters * per_iter * 32 * 32 * 2 * 2;
  const char* form = FORM == 0 ? "pk_fma" : FORM == 1 ? "x 2 v_fma_f32" : FORM == 2 ? "x 2 v_sub_f32" : "v_pk_fma_f32 (asm)";
  printf("2 waves/SIMD, %d accumulators, %d %s per MFMA: %.1f TFLOP/s\n", NACC, NVALU, form, flops / ms / 1e9);
}

int main() {
  int cus = 0;
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  float* out;
  (void)hipMalloc(&out, sizeof(float) * 256 * cus * 8);
  run<1, 0>(out, cus); run<2, 0>(out, cus); run<4, 0>(out, cus); run<8, 0>(out, cus);
  run<2, 1>(out, cus); run<2, 2>(out, cus); run<2, 4>(out, cus); run<2, 8>(out, cus);
  run<4, 2>(out, cus); run<4, 4>(out, cus); run<8, 2>(out, cus); run<8, 4>(out, cus);
  // the packed op itself, then the scalar columns: the same arithmetic as two scalar ops per packed one
  run<2, 1, 3>(out, cus); run<2, 2, 3>(out, cus); run<2, 4, 3>(out, cus); run<2, 8, 3>(out, cus);
  run<2, 1, 1>(out, cus); run<2, 2, 1>(out, cus); run<2, 4, 1>(out, cus); run<2, 8, 1>(out, cus);
  run<2, 1, 2>(out, cus); run<2, 2, 2>(out, cus); run<2, 4, 2>(out, cus); run<2, 8, 2>(out, cus);
  return 0;
}
