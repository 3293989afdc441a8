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
#include "logit_keys.h"

namespace pha {
namespace smp {

using namespace lk;

constexpr int MAX_B = 16;

typedef lk::Found<true> Found;

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

  // ---- stage the row as keys, find the largest (block_max's barrier publishes the zeroes too) ---
  const unsigned short* src = reinterpret_cast<const unsigned short*>(logits + (long)row * ld);
  unsigned kmax = stage_keys(src, keys, V, vec);
  for (int b = tid; b < L1_BINS; b += THREADS) { sm.cnt1[b] = 0u; sm.mass1[b] = 0ull; }
  if (tid == 0) { sm.found.mass_above = 0ull; sm.found.count_above = 0u; sm.found.bin = 0; sm.tok = 0; }
  kmax = block_max(kmax, sm.kmax, lane, wid);
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
    const Found f1 = scan_find<true>(sm.cnt1, sm.mass1, L1_BINS, false, (u64)K, sm.wt, &sm.found);
    hist2<T>(keys, V, (unsigned)f1.bin, filter_p, xmax, inv_t, sm);
    const Found f2 = scan_find<true>(sm.cnt2, sm.mass2, L2_BINS, false, (u64)K - f1.count_above, sm.wt, &sm.found);
    kt = ((unsigned)f1.bin << L2_BITS) | (unsigned)f2.bin;
    rt = (u64)K - f1.count_above - f2.count_above;
    ck = f1.mass_above + f2.mass_above + rt * qfix<T>(kt, xmax, inv_t);   // the mass top-k keeps
  }
  if (filter_p) {
    const double want = (double)top_p * (double)ck;
    u64 target = (u64)want;
    if ((double)target < want) ++target;
    target = target < 1 ? 1 : (target > ck ? ck : target);
    const Found f1 = scan_find<true>(sm.cnt1, sm.mass1, L1_BINS, true, target, sm.wt, &sm.found);
    hist2<T>(keys, V, (unsigned)f1.bin, true, xmax, inv_t, sm);
    const Found f2 = scan_find<true>(sm.cnt2, sm.mass2, L2_BINS, true, target - f1.mass_above, sm.wt, &sm.found);
    const unsigned kp = ((unsigned)f1.bin << L2_BITS) | (unsigned)f2.bin;
    const u64 above = f1.mass_above + f2.mass_above, qe = qfix<T>(kp, xmax, inv_t);
    u64 rp = (target > above && qe > 0) ? (target - above + qe - 1) / qe : 1;
    if (filter_k && kp == kt && rp > rt) rp = rt;   // never more than top-k left
    kt = kp;
    rt = rp < 1 ? 1 : rp;
  }
  const u64 qeq = qfix<T>(kt, xmax, inv_t);

  // ---- the draw, in ascending token index: thread t owns one contiguous chunk --------------------
  const Chunk ch = row_chunk(V);
  const int i0 = ch.i0, i1 = ch.i1;
  unsigned ties = 0u;
  u64 mgt = 0;
  for (int i = i0; i < i1; ++i) {
    const unsigned k = keys[i];
    if (k > kt) mgt += qfix<T>(k, xmax, inv_t);
    else if (k == kt) ++ties;
  }
  u64 tot_ties, M;
  const u64 tb = block_scan((u64)ties, sm.wt, &tot_ties);
  const u64 take = ties_taken(tb, ties, rt);
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
  static bool attr = false;
  size_t lds;
  int vec;
  const int e = keyed_launch(sample_kernel<T>, attr, sizeof(Smem), logits, ld, V, &lds, &vec);
  if (e != (int)hipSuccess) return e;
  hipLaunchKernelGGL(sample_kernel<T>, dim3(B), dim3(THREADS), lds, st, (const T*)logits, ld, u, ids, logprob, finished,
                     V, 1.f / temperature, top_k, top_p, eos, pad, vec);
  return (int)hipGetLastError();
}

}  // namespace smp
}  // namespace pha

// the largest vocabulary a row may have (its keys and the histograms share one workgroup's LDS)
PHA_API int pha_sample_logits_max_v() { return pha::lk::MAX_V; }

// logits [B, V] bf16 / fp16 with row stride ld (elements) and unit inner stride, u [B] fp32 in [0, 1),
// ids [B] int64, logprob [B] fp32, finished [B] bytes or null (read, and set where the row returns eos).
PHA_API int pha_sample_logits(int dt, const void* logits, long ld, const float* u, int64_t* ids, float* logprob,
                              unsigned char* finished, int B, int V, float temperature, int top_k, float top_p,
                              long eos, long pad, hipStream_t stream) {
  if (!logits || !u || !ids || !logprob) return (int)hipErrorInvalidValue;
  if (B < 1 || B > pha::smp::MAX_B || V < 2 || V > pha::lk::MAX_V || ld < V) return (int)hipErrorInvalidValue;
  if (!(temperature > 0.f) || !(top_p > 0.f) || top_p > 1.f || top_k < 0 || top_k > V) return (int)hipErrorInvalidValue;
  if (dt == pha::kBF16)
    return pha::smp::launch<pha::bf16_t>(logits, ld, u, ids, logprob, finished, B, V, temperature, top_k, top_p, eos,
                                         pad, stream);
  if (dt == pha::kF16)
    return pha::smp::launch<pha::half_t>(logits, ld, u, ids, logprob, finished, B, V, temperature, top_k, top_p, eos,
                                         pad, stream);
  return (int)hipErrorInvalidValue;
}
