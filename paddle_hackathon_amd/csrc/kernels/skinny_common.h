// What the weight-streaming GEMMs (skinny_gemm.hip: bf16 / fp16 weights, skinny_w8.hip: int8 weights)
// share: the MFMA fragment helpers, the epilogue (per-channel scale for int8 weights, bias, erf-GELU /
// tanh-GELU / ReLU, residual, one rounding), the store of an accumulator tile to the split-K workspace
// or through the epilogue, the finish kernel that sums the splits in a fixed order, and the split plan.
#pragma once
#include "mfma_tile.h"

namespace pha {
namespace sk {

using g256::f32x4;
using g256::Mf;

constexpr int MAX_M = 16;
constexpr int TARGET_WAVES = 1024;            // 4 streaming waves on each of 256 CUs
constexpr int MAX_SPLIT = 32;
constexpr int FIN_Q = 32, FIN_J = 8, FIN_THREADS = FIN_Q * FIN_J;

enum Act : int { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2, ACT_GELU_TANH = 3 };
enum Layout : int { LAYOUT_KN = 0, LAYOUT_NK = 1 };

// fragments stay in a native vector type (selects and array elements of it live in registers)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 ld16(const void* p) { return *reinterpret_cast<const u32x4*>(p); }
template <typename T>
__device__ __forceinline__ f32x4 mma(const u32x4& a, const u32x4& b, const f32x4& c) {
  return Mf<T>::mma(__builtin_bit_cast(uint4, a), __builtin_bit_cast(uint4, b), c);
}

__device__ __forceinline__ float act_apply(float v, int act) {
  if (act == ACT_GELU) return 0.5f * v * (1.f + erff(v * 0.7071067811865476f));
  if (act == ACT_RELU) return fmaxf(v, 0.f);
  if (act == ACT_GELU_TANH) {   // gelu_f(x, approx) of ce_gelu_embed.hip: what the GPT MLP trains with
    const float u = 0.7978845608028654f * (v + 0.044715f * v * v * v);
    const float th = 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * u) + 1.f);
    return 0.5f * v * (1.f + th);
  }
  return v;
}

template <typename T>
__device__ __forceinline__ void epi_store(float v, T* __restrict__ out, const T* __restrict__ bias,
                                          const T* __restrict__ res, int act, int m, int n, int N,
                                          const float* __restrict__ scale = nullptr) {
  const long i = (long)m * N + n;
  if (scale) v *= scale[n];                      // int8 weights: the channel's scale on the fp32 sum, before the bias
  if (bias) v += Cvt<T>::ld(bias, n);
  v = act_apply(v, act);
  if (res) v += Cvt<T>::ld(res, i);
  Cvt<T>::st(out, i, v);
}

// accumulator tile -> ws[s] or, fused, the epilogue. C/D map: col = lane & 15, row = 4 (lane >> 4) + j
template <typename T>
__device__ __forceinline__ void tile_store(const f32x4& acc, int col, int g, int s, bool fused, T* __restrict__ out,
                                           const T* __restrict__ bias, const T* __restrict__ res,
                                           float* __restrict__ ws, int act, int M, int N,
                                           const float* __restrict__ scale = nullptr) {
  if (col >= N) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = g * 4 + j;
    if (row < M) {
      if (fused) epi_store<T>(acc[j], out, bias, res, act, row, col, N, scale);
      else ws[((long)s * M + row) * N + col] = acc[j];
    }
  }
}

// Block = FIN_Q column quads x FIN_J split lanes. Lane j of a quad sums the splits j, j + FIN_J, ...
// (independent loads, all in flight at once), the lanes meet in LDS and lane 0 adds them in lane
// order: a fixed order that depends on nsplit alone. Then the epilogue on 4 columns of one row.
// SCALED (int8 weights): the sums are of unscaled partials and ``scale`` [N] multiplies them first.
template <typename T, bool SCALED>
__global__ __launch_bounds__(FIN_THREADS) void skinny_finish(const float* __restrict__ ws, const T* __restrict__ bias,
                                                             const T* __restrict__ res, T* __restrict__ out, int M,
                                                             int N, int nsplit, int act,
                                                             const float* __restrict__ scale) {
  __shared__ float4 part[FIN_J][FIN_Q];
  const int q = threadIdx.x % FIN_Q, j = threadIdx.x / FIN_Q;
  const long MN = (long)M * N;
  const long i = ((long)blockIdx.x * FIN_Q + q) * 4;
  const bool live = i < MN;                                   // MN % 4 == 0: a quad is wholly inside or outside
  const int m = live ? (int)(i / N) : 0, n = live ? (int)(i - (long)m * N) : 0;   // N % 4 == 0: one row per quad
  float bv[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f}, sv[4] = {1.f, 1.f, 1.f, 1.f};
  if (live && j == 0) {                                       // issued ahead of the partials' round trip
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (SCALED) sv[c] = scale[n + c];
      if (bias) bv[c] = Cvt<T>::ld(bias, n + c);
      if (res) rv[c] = Cvt<T>::ld(res, i + c);
    }
  }
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
#pragma unroll 4
    for (int s = j; s < nsplit; s += FIN_J) {
      const float4 p = *reinterpret_cast<const float4*>(ws + (long)s * MN + i);
      v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
  }
  part[j][q] = v;
  __syncthreads();
  if (!live || j != 0) return;
#pragma unroll
  for (int jj = 1; jj < FIN_J; ++jj) {
    const float4 p = part[jj][q];
    v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
  }
  const float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) Cvt<T>::st(out, i + c, act_apply((SCALED ? o[c] * sv[c] : o[c]) + bv[c], act) + rv[c]);
}

// (N, K) and the kernel's tile only: never M, never data, so a captured graph stays valid and results
// reproduce. As many K splits as bring the grid to TARGET_WAVES, each a multiple of the K step.
static inline void plan_tiles(int N, int K, int bn, int kstep, int* nsplit, int* kps) {
  const int tiles = (N + bn - 1) / bn;
  int ns = (TARGET_WAVES + tiles - 1) / tiles;
  const int most = K / kstep < 1 ? 1 : K / kstep;
  if (ns > most) ns = most;
  if (ns > MAX_SPLIT) ns = MAX_SPLIT;
  if (ns < 1) ns = 1;
  const int per = (K + ns - 1) / ns;
  *kps = (per + kstep - 1) / kstep * kstep;
  *nsplit = (K + *kps - 1) / *kps;
}

}  // namespace sk
}  // namespace pha
