// Weight-streaming GEMM for 1 <= M <= 16 rows (the decode step's four products per layer):
//   out[M, N] = act(x[M, K] . W + bias[N]) + residual[M, N],  bf16 / fp16 operands, fp32 accumulation.
//
// Every weight byte is used once, so the weights go global -> VGPR in 16-byte loads with many in
// flight per wave and one late wait; x (at most 256 KB, L2-resident) is loaded in MFMA fragment
// shape. The product is one 16-row block of mfma_f32_16x16x32: lanes whose row is >= M keep zeros
// and load nothing, and since an MFMA row depends on its own A row alone, row i of the result does
// not depend on M. One workgroup is one wave: it owns a column tile and one K split, no barrier
// joins it to any other wave.
//
//  * W stored [N, K] (skinny_nk): lane (n = lane & 15, g = lane >> 4) loads the 16 bytes at
//    W[n][k + 32u + 8g], which IS its B fragment of MFMA u; a wave instruction reads 64 contiguous
//    bytes of 16 rows and the 8 instructions of a K step cover adjacent pieces, so every fetched
//    line is used in full. x is loaded at the same k, two column tiles share each x fragment.
//  * W stored [K, N] (skinny_kn): the B fragment is k-strided, so the wave loads full 128-byte row
//    pieces (8 k-rows x 64 columns per instruction, 16 in flight), writes them to a [128 k][64 n]
//    LDS image of its own and reads the fragments back transposed with ds_read_b64_tr_b16 (the
//    attention kernels' V recipe, mfma_tile.h tn_frag).
//
// Split-K is deterministic: the plan depends on (N, K, layout) alone, split s writes its fp32
// partial to ws[s, M, N] with plain stores, and skinny_finish sums the splits in a fixed order and
// applies the epilogue (bias, erf-GELU / tanh-GELU / ReLU, residual, one rounding). With one split the
// first kernel applies the epilogue itself. No atomics; two plain launches on the caller's stream.
//
// Tails: N % 8 == K % 8 == 0, so a 16-byte piece is wholly inside or outside. Column pieces
// outside N load a clamped (valid) address and their results are never stored; k pieces outside
// the split load a clamped address and are replaced by zeros in registers in both operands.
#include "mfma_tile.h"

namespace pha {
namespace sk {

using g256::f32x4;
using g256::Mf;

constexpr int MAX_M = 16;
constexpr int NK_BN = 32, NK_KSTEP = 256;     // [N, K]: 2 column tiles x 8 MFMA k-steps per iteration
constexpr int KN_BN = 64, KN_KSTEP = 128;     // [K, N]: 4 column tiles x 4 MFMA k-steps per iteration
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
                                          const T* __restrict__ res, int act, int m, int n, int N) {
  const long i = (long)m * N + n;
  if (bias) v += Cvt<T>::ld(bias, n);
  v = act_apply(v, act);
  if (res) v += Cvt<T>::ld(res, i);
  Cvt<T>::st(out, i, v);
}

// accumulator tile -> ws[s] or, fused, the epilogue. C/D map: col = lane & 15, row = 4 (lane >> 4) + j
template <typename T>
__device__ __forceinline__ void tile_store(const f32x4& acc, int col, int g, int s, bool fused, T* __restrict__ out,
                                           const T* __restrict__ bias, const T* __restrict__ res,
                                           float* __restrict__ ws, int act, int M, int N) {
  if (col >= N) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = g * 4 + j;
    if (row < M) {
      if (fused) epi_store<T>(acc[j], out, bias, res, act, row, col, N);
      else ws[((long)s * M + row) * N + col] = acc[j];
    }
  }
}

template <typename T, bool TAIL>
__device__ __forceinline__ void nk_step(const T* __restrict__ xr, const T* __restrict__ w0, const T* __restrict__ w1,
                                        bool rowok, int k, int kend, int g, f32x4& acc0, f32x4& acc1) {
  constexpr int U = NK_KSTEP / 32;
  const u32x4 z = {0u, 0u, 0u, 0u};
  u32x4 a[U], b0[U], b1[U];
  int kc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int kk = k + 32 * u + 8 * g;
    kc[u] = TAIL ? min(kk, kend - 8) : kk;       // clamped: always a piece inside the split
    b0[u] = ld16(w0 + kc[u]);
    b1[u] = ld16(w1 + kc[u]);
    a[u] = z;
  }
  if (rowok) {                                   // rows >= M stay zero and are never loaded
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = ld16(xr + kc[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (TAIL) {
      const bool ok = k + 32 * u + 8 * g < kend;
      a[u] = ok ? a[u] : z;
      b0[u] = ok ? b0[u] : z;
      b1[u] = ok ? b1[u] : z;
    }
    acc0 = mma<T>(a[u], b0[u], acc0);
    acc1 = mma<T>(a[u], b1[u], acc1);
  }
}

// W [N, K]. grid (ceil(N / NK_BN), nsplit), one wave per workgroup.
template <typename T>
__global__ __launch_bounds__(64) void skinny_nk(const T* __restrict__ x, long ldx, const T* __restrict__ W,
                                                const T* __restrict__ bias, const T* __restrict__ res,
                                                T* __restrict__ out, float* __restrict__ ws, int M, int N, int K,
                                                int kps, int act, int fused) {
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * NK_BN, s = blockIdx.y;
  const int kbeg = s * kps, kend = min(kbeg + kps, K);
  const T* w0 = W + (long)min(n0 + r, N - 1) * K;        // a column past N reads row N - 1, never stored
  const T* w1 = W + (long)min(n0 + 16 + r, N - 1) * K;
  const bool rowok = r < M;
  const T* xr = x + (long)(rowok ? r : 0) * ldx;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int k = kbeg;
  for (; k + NK_KSTEP <= kend; k += NK_KSTEP) nk_step<T, false>(xr, w0, w1, rowok, k, kend, g, acc0, acc1);
  if (k < kend) nk_step<T, true>(xr, w0, w1, rowok, k, kend, g, acc0, acc1);
  tile_store<T>(acc0, n0 + r, g, s, fused != 0, out, bias, res, ws, act, M, N);
  tile_store<T>(acc1, n0 + 16 + r, g, s, fused != 0, out, bias, res, ws, act, M, N);
}

template <typename T, bool TAIL>
__device__ __forceinline__ void kn_step(const T* __restrict__ xr, const T* __restrict__ wp, long N, bool rowok,
                                        unsigned char* img, int k, int kend, int lane, f32x4 (&acc)[4]) {
  constexpr int U = KN_KSTEP / 8, KS = KN_KSTEP / 32;
  const u32x4 z = {0u, 0u, 0u, 0u};
  const int r = lane & 15, g = lane >> 4, lr = lane >> 3, lc = lane & 7;
  u32x4 w[U], a[KS];
  int kc[KS];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int kr = k + 8 * u + lr;
    w[u] = ld16(wp + (long)(TAIL ? min(kr, kend - 1) : kr) * N);
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int kk = k + 32 * ks + 8 * g;
    kc[ks] = TAIL ? min(kk, kend - 8) : kk;
    a[ks] = z;
  }
  if (rowok) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a[ks] = ld16(xr + kc[ks]);
  }
  __syncthreads();                               // one wave: orders the image's reuse for the compiler
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int row = 8 * u + lr;
    if (TAIL) w[u] = (k + row < kend) ? w[u] : z;
    *reinterpret_cast<u32x4*>(img + row * 128 + ((lc ^ g256::tn_mask(row, 128)) << 4)) = w[u];
  }
  __syncthreads();
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    if (TAIL) a[ks] = (k + 32 * ks + 8 * g < kend) ? a[ks] : z;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint4 b = g256::tn_frag<128>(img, 32 * ks + 8 * g, 16 * t, r >> 2, r & 3);
      acc[t] = Mf<T>::mma(__builtin_bit_cast(uint4, a[ks]), b, acc[t]);
    }
  }
}

// W [K, N]. grid (ceil(N / KN_BN), nsplit), one wave per workgroup, 16 KB of LDS.
template <typename T>
__global__ __launch_bounds__(64) void skinny_kn(const T* __restrict__ x, long ldx, const T* __restrict__ W,
                                                const T* __restrict__ bias, const T* __restrict__ res,
                                                T* __restrict__ out, float* __restrict__ ws, int M, int N, int K,
                                                int kps, int act, int fused) {
  __shared__ __attribute__((aligned(16))) unsigned char img[KN_KSTEP * 128];
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * KN_BN, s = blockIdx.y;
  const int kbeg = s * kps, kend = min(kbeg + kps, K);
  const int nc = n0 + 8 * (lane & 7);
  const T* wp = W + (nc < N ? nc : 0);           // a column piece past N reads columns 0..7, never stored
  const bool rowok = r < M;
  const T* xr = x + (long)(rowok ? r : 0) * ldx;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  int k = kbeg;
  for (; k + KN_KSTEP <= kend; k += KN_KSTEP) kn_step<T, false>(xr, wp, N, rowok, img, k, kend, lane, acc);
  if (k < kend) kn_step<T, true>(xr, wp, N, rowok, img, k, kend, lane, acc);
#pragma unroll
  for (int t = 0; t < 4; ++t) tile_store<T>(acc[t], n0 + 16 * t + r, g, s, fused != 0, out, bias, res, ws, act, M, N);
}

// Block = FIN_Q column quads x FIN_J split lanes. Lane j of a quad sums the splits j, j + FIN_J, ...
// (independent loads, all in flight at once), the lanes meet in LDS and lane 0 adds them in lane
// order: a fixed order that depends on nsplit alone. Then the epilogue on 4 columns of one row.
template <typename T>
__global__ __launch_bounds__(FIN_THREADS) void skinny_finish(const float* __restrict__ ws, const T* __restrict__ bias,
                                                             const T* __restrict__ res, T* __restrict__ out, int M,
                                                             int N, int nsplit, int act) {
  __shared__ float4 part[FIN_J][FIN_Q];
  const int q = threadIdx.x % FIN_Q, j = threadIdx.x / FIN_Q;
  const long MN = (long)M * N;
  const long i = ((long)blockIdx.x * FIN_Q + q) * 4;
  const bool live = i < MN;                                   // MN % 4 == 0: a quad is wholly inside or outside
  const int m = live ? (int)(i / N) : 0, n = live ? (int)(i - (long)m * N) : 0;   // N % 4 == 0: one row per quad
  float bv[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f};
  if (live && j == 0) {                                       // issued ahead of the partials' round trip
#pragma unroll
    for (int c = 0; c < 4; ++c) {
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
  for (int c = 0; c < 4; ++c) Cvt<T>::st(out, i + c, act_apply(o[c] + bv[c], act) + rv[c]);
}

static void tile_of(int layout, int* bn, int* kstep) {
  *bn = layout == LAYOUT_NK ? NK_BN : KN_BN;
  *kstep = layout == LAYOUT_NK ? NK_KSTEP : KN_KSTEP;
}

// (N, K, layout) only: never M, never data, so a captured graph stays valid and results reproduce
static void plan(int N, int K, int layout, int* nsplit, int* kps) {
  int bn, kstep;
  tile_of(layout, &bn, &kstep);
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

template <typename T>
static int launch(int layout, const void* x, long ldx, const void* w, const void* bias, const void* res, void* out,
                  float* ws, int M, int N, int K, int nsplit, int kps, int act, hipStream_t st) {
  int bn, kstep;
  tile_of(layout, &bn, &kstep);
  const dim3 grid((N + bn - 1) / bn, nsplit);
  const int fused = nsplit == 1;
  if (layout == LAYOUT_NK)
    skinny_nk<T><<<grid, 64, 0, st>>>((const T*)x, ldx, (const T*)w, (const T*)bias, (const T*)res, (T*)out, ws, M, N,
                                      K, kps, act, fused);
  else
    skinny_kn<T><<<grid, 64, 0, st>>>((const T*)x, ldx, (const T*)w, (const T*)bias, (const T*)res, (T*)out, ws, M, N,
                                      K, kps, act, fused);
  if (!fused) {
    const long quads = (long)M * N / 4;
    skinny_finish<T><<<(unsigned)((quads + FIN_Q - 1) / FIN_Q), FIN_THREADS, 0, st>>>(
        ws, (const T*)bias, (const T*)res, (T*)out, M, N, nsplit, act);
  }
  return (int)hipGetLastError();
}

}  // namespace sk
}  // namespace pha

// the kernel's column tile and per-iteration K step for a layout (1: W [N, K], 0: W [K, N])
PHA_API int pha_skinny_gemm_tile(int layout, int* col_tile, int* k_step) {
  if ((layout != 0 && layout != 1) || !col_tile || !k_step) return (int)hipErrorInvalidValue;
  pha::sk::tile_of(layout, col_tile, k_step);
  return 0;
}

PHA_API int pha_skinny_gemm_plan(int N, int K, int layout, int* nsplit, int* k_per_split) {
  if (N <= 0 || K <= 0 || (layout != 0 && layout != 1) || !nsplit || !k_per_split) return (int)hipErrorInvalidValue;
  pha::sk::plan(N, K, layout, nsplit, k_per_split);
  return 0;
}

// x [M, K] with row stride ldx (elements), w [N, K] (layout 1) or [K, N] (layout 0), bias [N] or null,
// residual [M, N] or null, out [M, N], ws fp32 [nsplit, M, N] (unused and may be null when nsplit == 1).
// Split s covers k in [s * k_per_split, min((s + 1) * k_per_split, K)); none may be empty.
PHA_API int pha_skinny_gemm(int dt, int layout, const void* x, long ldx, const void* w, const void* bias,
                            const void* residual, void* out, float* ws, int M, int N, int K, int nsplit,
                            int k_per_split, int act, hipStream_t stream) {
  if (M < 1 || M > pha::sk::MAX_M || N < 8 || K < 8 || N % 8 || K % 8 || ldx < K || ldx % 8) return (int)hipErrorInvalidValue;
  if ((layout != 0 && layout != 1) || act < 0 || act > 3 || !x || !w || !out) return (int)hipErrorInvalidValue;
  if (nsplit < 1 || nsplit > 65535 || k_per_split < 8 || k_per_split % 8) return (int)hipErrorInvalidValue;
  if ((long)(nsplit - 1) * k_per_split >= K || (long)nsplit * k_per_split < K) return (int)hipErrorInvalidValue;
  if (nsplit > 1 && !ws) return (int)hipErrorInvalidValue;
  if (dt == pha::kBF16)
    return pha::sk::launch<pha::bf16_t>(layout, x, ldx, w, bias, residual, out, ws, M, N, K, nsplit, k_per_split, act,
                                        stream);
  if (dt == pha::kF16)
    return pha::sk::launch<pha::half_t>(layout, x, ldx, w, bias, residual, out, ws, M, N, K, nsplit, k_per_split, act,
                                        stream);
  return (int)hipErrorInvalidValue;
}
