// What the keyed-histogram kernels share (sampling.hip, beam_search.hip): one workgroup of 1024 threads
// owns one row of 16-bit logits, stages it in LDS as 16-bit order-preserving keys and finds the k-th
// key (or a mass boundary) with two histogram levels over the key, its upper 11 bits and then the
// lower 5 inside the boundary bin. A token's probability enters every sum as the integer qfix().
// Both kernels score a token through these definitions, which is what makes a one-beam step and a
// greedy step agree bit for bit.
#pragma once
#include "common.h"

namespace pha {
namespace lk {

typedef unsigned long long u64;

constexpr int THREADS = 1024, WAVES = THREADS / 64;
constexpr int MAX_V = 65536;   // a row's keys and the histograms share one workgroup's LDS
constexpr int L2_BITS = 5, L1_BINS = 1 << (16 - L2_BITS), L2_BINS = 1 << L2_BITS;
constexpr float FIX_ONE = 1099511627776.f;   // 2^40

// larger logit <=> larger key; -0 and +0 are one logit and get one key
__device__ __forceinline__ unsigned key_of(unsigned b) {
  if ((b & 0x7fffu) == 0u) b = 0u;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
template <typename T> __device__ __forceinline__ float val_of(unsigned key);
template <> __device__ __forceinline__ float val_of<bf16_t>(unsigned key) {
  const unsigned b = (key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xffffu);
  return bf16_to_f32((uint16_t)b);
}
template <> __device__ __forceinline__ float val_of<half_t>(unsigned key) {
  const unsigned b = (key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xffffu);
  return (float)__builtin_bit_cast(_Float16, (uint16_t)b);
}

// the mass of a token in 2^-40 units of the largest one: a pure function of (key, xmax, inv_t)
template <typename T>
__device__ __forceinline__ u64 qfix(unsigned key, float xmax, float inv_t) {
  return (u64)(__expf((val_of<T>(key) - xmax) * inv_t) * FIX_ONE);
}

// exclusive prefix of v over the block in thread order, and the block's total; ends on a barrier
__device__ __forceinline__ u64 block_scan(u64 v, u64* wt, u64* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  u64 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  if (lane == 63) wt[wid] = inc;
  __syncthreads();
  u64 base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const u64 x = wt[w];
    if (w < wid) base += x;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// Stage the row `src` [V] in LDS as keys and return the largest this thread saw. Global loads are 16
// bytes per lane where `vec` says the row base is 16-byte aligned, scalar otherwise; elements past V
// are never read. The kernels zero their histograms between this and block_max, while the loads are
// in flight: a separate step from block_max so that this order compiles as it always did.
__device__ __forceinline__ unsigned stage_keys(const unsigned short* src, unsigned short* keys, int V, int vec) {
  const int tid = threadIdx.x;
  unsigned kmax = 0u;
  const int vend = vec ? (V & ~7) : 0;
  for (int c = tid * 8; c < vend; c += THREADS * 8) {
    const uint4 r = *reinterpret_cast<const uint4*>(src + c);
    unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned lo = key_of(w[j] & 0xffffu), hi = key_of(w[j] >> 16);
      kmax = max(kmax, max(lo, hi));
      w[j] = lo | (hi << 16);
    }
    *reinterpret_cast<uint4*>(keys + c) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  for (int c = vend + tid; c < V; c += THREADS) {
    const unsigned k = key_of(src[c]);
    kmax = max(kmax, k);
    keys[c] = (unsigned short)k;
  }
  return kmax;
}

// the block's largest key through kmax_w (WAVES words of LDS); its one barrier also publishes the staged
// keys and whatever else the caller wrote to LDS before the call. lane, wid: the caller's tid & 63 and
// tid >> 6 (formed here again they cost an instruction the in-place code did not have)
__device__ __forceinline__ unsigned block_max(unsigned kmax, unsigned* kmax_w, int lane, int wid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64));
  if (lane == 0) kmax_w[wid] = kmax;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WAVES; ++w) kmax = max(kmax, kmax_w[w]);
  return kmax;
}

// the bin a scan stopped in, and what lies in the bins above it (the mass only where it is scanned)
// count_t: the width scan_find holds a bin's count in, each kernel's own (profiles/generate/README.md)
template <bool MASS> struct Found;
template <> struct Found<true> {
  typedef unsigned count_t;
  u64 mass_above;
  unsigned count_above;
  int bin;
};
template <> struct Found<false> {
  typedef u64 count_t;
  unsigned count_above;
  int bin;
};

// Walk the bins from the highest down and stop in the one where the running count (with MASS and
// by_mass: the running mass) first reaches target: 1 <= target <= the total. Thread t owns the bins at
// descending positions 2t, 2t + 1. Without MASS `mass` is not read and there is one block_scan.
// wt: WAVES words of LDS; slot: one Found in LDS, zeroed before the first call.
template <bool MASS>
__device__ __forceinline__ Found<MASS> scan_find(const unsigned* cnt, const u64* mass, int nbins, bool by_mass,
                                                 u64 target, u64* wt, Found<MASS>* slot) {
  const int b0 = nbins - 1 - 2 * (int)threadIdx.x, b1 = b0 - 1;
  typename Found<MASS>::count_t c0 = 0, c1 = 0;
  u64 m0 = 0, m1 = 0;
  if (b0 >= 0) { c0 = cnt[b0]; if constexpr (MASS) m0 = mass[b0]; }
  if (b1 >= 0) { c1 = cnt[b1]; if constexpr (MASS) m1 = mass[b1]; }
  u64 tot, em = 0;
  const u64 ec = block_scan((u64)c0 + c1, wt, &tot);
  if constexpr (MASS) em = block_scan(m0 + m1, wt, &tot);
  const bool bm = MASS && by_mass;
  const u64 e = bm ? em : ec, v0 = bm ? m0 : (u64)c0, v1 = bm ? m1 : (u64)c1;
  if (b0 >= 0 && e < target && target <= e + v0) {
    if constexpr (MASS) slot->mass_above = em;
    slot->count_above = (unsigned)ec; slot->bin = b0;
  } else if (b1 >= 0 && e + v0 < target && target <= e + v0 + v1) {
    if constexpr (MASS) slot->mass_above = em + m0;
    slot->count_above = (unsigned)ec + c0; slot->bin = b1;
  }
  __syncthreads();
  const Found<MASS> f = *slot;
  __syncthreads();
  return f;
}

// The last pass walks the row in ascending token index: thread t owns the contiguous chunk [i0, i1).
struct Chunk {
  int i0, i1;
};
__device__ __forceinline__ Chunk row_chunk(int V) {
  int chunk = (V + THREADS - 1) / THREADS;
  chunk += (6 - (chunk & 3)) & 3;   // chunk % 4 == 2: an odd stride in LDS words, no bank conflict
  const int i0 = min((int)threadIdx.x * chunk, V);
  return {i0, min(i0 + chunk, V)};
}

// Of the tokens whose key equals the boundary key the first rt (by index) stay: how many of this
// thread's `ties`, given the tb such tokens in the chunks before it.
__device__ __forceinline__ u64 ties_taken(u64 tb, unsigned ties, u64 rt) {
  return tb >= rt ? 0 : (rt - tb < (u64)ties ? rt - tb : (u64)ties);
}

// Host side of a launch of `kernel`, whose LDS is `smem` bytes of its own and the row's keys behind
// them: raises the kernel's dynamic-LDS limit once (`latch`, one per kernel) and gives the launch its
// LDS size and whether the row base allows 16-byte loads. Returns a hipError_t.
template <typename Kernel>
static int keyed_launch(Kernel* kernel, bool& latch, size_t smem, const void* logits, long ld, int V, size_t* lds,
                        int* vec) {
  if (!latch) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(smem + 2 * MAX_V));
    if (e != hipSuccess) return (int)e;
    latch = true;
  }
  *lds = smem + 2 * (size_t)((V + 7) / 8 * 8);
  *vec = ((uintptr_t)logits % 16 == 0 && ld % 8 == 0) ? 1 : 0;
  return (int)hipSuccess;
}

}  // namespace lk
}  // namespace pha
