// Next-token sampling for the decode step: logits [B, V] (bf16 / fp16) -> token ids and their log
// probabilities, with temperature, top-k, top-p, the multinomial draw and the EOS bookkeeping in one
// launch. One workgroup of 1024 threads owns one row.
//
// Contract (the float64 reference in tests/test_sample_logits_gpu.py spells out the same):
//   p = softmax(logits / temperature); order = stable descending sort by logit (ties: lower index
//   first); top-k keeps the first k of the order; top-p keeps the shortest prefix of what top-k left
//   whose mass, renormalised over it, reaches top_p (at least one token); the kept set is walked in
//   ascending token index and the first token whose running mass exceeds u * (kept mass) is returned.
//   top_k == 1 returns the argmax (lowest index on a tie) and ignores u.
//
// No sort: a 16-bit logit has a 16-bit order-preserving key, so the k-th logit and the top-p boundary
// are found by two histogram levels over the key (its upper 11 bits, then the lower 5 inside the
// boundary bin) that carry a count and a mass per bin. Tokens that share the boundary key share one
// probability; how many of them stay follows from arithmetic, and which (the lowest indices) from an
// index-ordered prefix count in the last pass.
//
// Bitwise reproducible: a probability enters every sum as the integer trunc(exp(z - zmax) * 2^40).
// Integer sums do not depend on the order of arrival, so the histogram masses (64-bit LDS atomics),
// the normaliser, the kept mass and the running mass of the draw are exact functions of the inputs;
// u is compared as floor(u * kept mass). A row has at most 2^16 tokens of mass at most 2^40 each.
//
// The row is staged once in LDS as keys (2 V bytes; 100 KB at V = 50,304) next to 25 KB of
// histograms, which is what bounds V at 65,536. Global loads are 16 bytes per lane where the row
// base is 16-byte aligned, scalar otherwise; elements past V are never read.
#include "common.h"

namespace pha {
namespace smp {

typedef unsigned long long u64;

constexpr int THREADS = 1024, WAVES = THREADS / 64;
constexpr int MAX_V = 65536, MAX_B = 16;
constexpr int L2_BITS = 5, L1_BINS = 1 << (16 - L2_BITS), L2_BINS = 1 << L2_BITS;
constexpr float FIX_ONE = 1099511627776.f;   // 2^40

// the bin a scan stopped in, and what lies in the bins above it
struct Found {
  u64 mass_above;
  unsigned count_above;
  int bin;
};

struct Smem {
  u64 mass1[L1_BINS];
  u64 mass2[L2_BINS];
  u64 wt[WAVES];
  Found found;
  unsigned cnt1[L1_BINS];
  unsigned cnt2[L2_BINS];
  unsigned kmax[WAVES];
  int tok;
  int pad_[3];
};
static_assert(sizeof(Smem) % 16 == 0, "the keys behind it are stored 16 bytes at a time");
static_assert(sizeof(Smem) + 2 * MAX_V <= 160 * 1024, "one workgroup's LDS");

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

// Walk the bins from the highest down and stop in the one where the running count (or mass) first
// reaches target: 1 <= target <= the total. Thread t owns the bins at descending positions 2t, 2t + 1.
__device__ __forceinline__ Found scan_find(const unsigned* cnt, const u64* mass, int nbins, bool by_mass, u64 target,
                                           Smem& sm) {
  const int b0 = nbins - 1 - 2 * (int)threadIdx.x, b1 = b0 - 1;
  unsigned c0 = 0, c1 = 0;
  u64 m0 = 0, m1 = 0;
  if (b0 >= 0) { c0 = cnt[b0]; m0 = mass[b0]; }
  if (b1 >= 0) { c1 = cnt[b1]; m1 = mass[b1]; }
  u64 totc, totm;
  const u64 ec = block_scan((u64)c0 + c1, sm.wt, &totc);
  const u64 em = block_scan(m0 + m1, sm.wt, &totm);
  const u64 e = by_mass ? em : ec, v0 = by_mass ? m0 : (u64)c0, v1 = by_mass ? m1 : (u64)c1;
  if (b0 >= 0 && e < target && target <= e + v0) {
    sm.found.mass_above = em; sm.found.count_above = (unsigned)ec; sm.found.bin = b0;
  } else if (b1 >= 0 && e + v0 < target && target <= e + v0 + v1) {
    sm.found.mass_above = em + m0; sm.found.count_above = (unsigned)ec + c0; sm.found.bin = b1;
  }
  __syncthreads();
  const Found f = sm.found;
  __syncthreads();
  return f;
}

// second level: the tokens whose upper key bits are `bin1`, by their lower L2_BITS
template <typename T>
__device__ __forceinline__ void hist2(const unsigned short* keys, int V, unsigned bin1, bool need_mass, float xmax,
                                      float inv_t, Smem& sm) {
  if (threadIdx.x < L2_BINS) { sm.cnt2[threadIdx.x] = 0u; sm.mass2[threadIdx.x] = 0ull; }
  __syncthreads();
  for (int i = threadIdx.x; i < V; i += THREADS) {
    const unsigned k = keys[i];
    if ((k >> L2_BITS) == bin1) {
      atomicAdd(&sm.cnt2[k & (L2_BINS - 1)], 1u);
      if (need_mass) atomicAdd(&sm.mass2[k & (L2_BINS - 1)], qfix<T>(k, xmax, inv_t));
    }
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(THREADS) void sample_kernel(const T* __restrict__ logits, long ld,
                                                         const float* __restrict__ u, int64_t* __restrict__ ids,
                                                         float* __restrict__ logprob,
                                                         unsigned char* __restrict__ finished, int V, float inv_t,
                                                         int top_k, float top_p, long eos, long pad, int vec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem& sm = *reinterpret_cast<Smem*>(smem_raw);
  unsigned short* keys = reinterpret_cast<unsigned short*>(smem_raw + sizeof(Smem));
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int row = blockIdx.x;
  if (finished && finished[row]) {   // the whole block takes this branch or none of it does
    if (tid == 0) { ids[row] = pad; logprob[row] = 0.f; }
    return;
  }
  const bool greedy = top_k == 1;
  const int K = (top_k > 0 && top_k < V) ? top_k : V;
  const bool filter_k = K < V && !greedy, filter_p = top_p < 1.f && !greedy;

  // ---- stage the row as keys, find the largest -------------------------------------------------
  const unsigned short* src = reinterpret_cast<const unsigned short*>(logits + (long)row * ld);
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
  for (int b = tid; b < L1_BINS; b += THREADS) { sm.cnt1[b] = 0u; sm.mass1[b] = 0ull; }
  if (tid == 0) { sm.found.mass_above = 0ull; sm.found.count_above = 0u; sm.found.bin = 0; sm.tok = 0; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64));
  if (lane == 0) sm.kmax[wid] = kmax;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WAVES; ++w) kmax = max(kmax, sm.kmax[w]);
  const float xmax = val_of<T>(kmax);

  // ---- the normaliser, and the first-level histogram where a filter needs it ----------------------
  u64 zloc = 0;
  for (int i = tid; i < V; i += THREADS) {
    const unsigned k = keys[i];
    const u64 q = qfix<T>(k, xmax, inv_t);
    zloc += q;
    if (filter_k || filter_p) {
      atomicAdd(&sm.cnt1[k >> L2_BITS], 1u);
      if (filter_p) atomicAdd(&sm.mass1[k >> L2_BITS], q);
    }
  }
  u64 Z;
  block_scan(zloc, sm.wt, &Z);   // its barriers also publish the histogram

  // ---- the threshold: keys above kt stay, and the first rt (by index) of those equal to it -------
  unsigned kt = 0u;
  u64 rt = (u64)V, ck = Z;
  if (greedy) {
    kt = kmax;
    rt = 1;
  }
  if (filter_k) {
    const Found f1 = scan_find(sm.cnt1, sm.mass1, L1_BINS, false, (u64)K, sm);
    hist2<T>(keys, V, (unsigned)f1.bin, filter_p, xmax, inv_t, sm);
    const Found f2 = scan_find(sm.cnt2, sm.mass2, L2_BINS, false, (u64)K - f1.count_above, sm);
    kt = ((unsigned)f1.bin << L2_BITS) | (unsigned)f2.bin;
    rt = (u64)K - f1.count_above - f2.count_above;
    ck = f1.mass_above + f2.mass_above + rt * qfix<T>(kt, xmax, inv_t);   // the mass top-k keeps
  }
  if (filter_p) {
    const double want = (double)top_p * (double)ck;
    u64 target = (u64)want;
    if ((double)target < want) ++target;
    target = target < 1 ? 1 : (target > ck ? ck : target);
    const Found f1 = scan_find(sm.cnt1, sm.mass1, L1_BINS, true, target, sm);
    hist2<T>(keys, V, (unsigned)f1.bin, true, xmax, inv_t, sm);
    const Found f2 = scan_find(sm.cnt2, sm.mass2, L2_BINS, true, target - f1.mass_above, sm);
    const unsigned kp = ((unsigned)f1.bin << L2_BITS) | (unsigned)f2.bin;
    const u64 above = f1.mass_above + f2.mass_above, qe = qfix<T>(kp, xmax, inv_t);
    u64 rp = (target > above && qe > 0) ? (target - above + qe - 1) / qe : 1;
    if (filter_k && kp == kt && rp > rt) rp = rt;   // never more than top-k left
    kt = kp;
    rt = rp < 1 ? 1 : rp;
  }
  const u64 qeq = qfix<T>(kt, xmax, inv_t);

  // ---- the draw, in ascending token index: thread t owns one contiguous chunk --------------------
  int chunk = (V + THREADS - 1) / THREADS;
  chunk += (6 - (chunk & 3)) & 3;   // chunk % 4 == 2: an odd stride in LDS words, no bank conflict
  const int i0 = min(tid * chunk, V), i1 = min(i0 + chunk, V);
  unsigned ties = 0u;
  u64 mgt = 0;
  for (int i = i0; i < i1; ++i) {
    const unsigned k = keys[i];
    if (k > kt) mgt += qfix<T>(k, xmax, inv_t);
    else if (k == kt) ++ties;
  }
  u64 tot_ties, M;
  const u64 tb = block_scan((u64)ties, sm.wt, &tot_ties);
  const u64 take = tb >= rt ? 0 : (rt - tb < (u64)ties ? rt - tb : (u64)ties);
  const u64 own = mgt + take * qeq;
  const u64 mb = block_scan(own, sm.wt, &M);
  u64 tu = 0;
  if (!greedy) {
    tu = (u64)((double)u[row] * (double)M);   // u < 1: tu < M
    if (M > 0 && tu >= M) tu = M - 1;
  }
  if (own > 0 && mb <= tu && tu < mb + own) {   // exactly one thread
    u64 run = mb, tr = tb;
    for (int i = i0; i < i1; ++i) {
      const unsigned k = keys[i];
      if (k > kt) run += qfix<T>(k, xmax, inv_t);
      else if (k == kt) { if (tr < rt) run += qeq; ++tr; }
      if (run > tu) { sm.tok = i; break; }
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int tok = min(max(sm.tok, 0), V - 1);
    const float zf = (float)Z * (1.f / FIX_ONE);
    ids[row] = tok;
    logprob[row] = (val_of<T>(keys[tok]) - xmax) * inv_t - logf(zf);
    if (finished && (long)tok == eos) finished[row] = 1;
  }
}

template <typename T>
static int launch(const void* logits, long ld, const float* u, int64_t* ids, float* logprob, unsigned char* finished,
                  int B, int V, float temperature, int top_k, float top_p, long eos, long pad, hipStream_t st) {
  const size_t lds = sizeof(Smem) + 2 * (size_t)((V + 7) / 8 * 8);
  static bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute((const void*)sample_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(sizeof(Smem) + 2 * MAX_V));
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  const int vec = ((uintptr_t)logits % 16 == 0 && ld % 8 == 0) ? 1 : 0;
  hipLaunchKernelGGL(sample_kernel<T>, dim3(B), dim3(THREADS), lds, st, (const T*)logits, ld, u, ids, logprob, finished,
                     V, 1.f / temperature, top_k, top_p, eos, pad, vec);
  return (int)hipGetLastError();
}

}  // namespace smp
}  // namespace pha

// the largest vocabulary a row may have (its keys and the histograms share one workgroup's LDS)
PHA_API int pha_sample_logits_max_v() { return pha::smp::MAX_V; }

// logits [B, V] bf16 / fp16 with row stride ld (elements) and unit inner stride, u [B] fp32 in [0, 1),
// ids [B] int64, logprob [B] fp32, finished [B] bytes or null (read, and set where the row returns eos).
PHA_API int pha_sample_logits(int dt, const void* logits, long ld, const float* u, int64_t* ids, float* logprob,
                              unsigned char* finished, int B, int V, float temperature, int top_k, float top_p,
                              long eos, long pad, hipStream_t stream) {
  if (!logits || !u || !ids || !logprob) return (int)hipErrorInvalidValue;
  if (B < 1 || B > pha::smp::MAX_B || V < 2 || V > pha::smp::MAX_V || ld < V) return (int)hipErrorInvalidValue;
  if (!(temperature > 0.f) || !(top_p > 0.f) || top_p > 1.f || top_k < 0 || top_k > V) return (int)hipErrorInvalidValue;
  if (dt == pha::kBF16)
    return pha::smp::launch<pha::bf16_t>(logits, ld, u, ids, logprob, finished, B, V, temperature, top_k, top_p, eos,
                                         pad, stream);
  if (dt == pha::kF16)
    return pha::smp::launch<pha::half_t>(logits, ld, u, ids, logprob, finished, B, V, temperature, top_k, top_p, eos,
                                         pad, stream);
  return (int)hipErrorInvalidValue;
}
