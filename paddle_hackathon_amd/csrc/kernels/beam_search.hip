// One beam-search step for the decode loop: logits [R, V] (bf16 / fp16), R = B * K rows in groups of
// K consecutive beams -> per row the next token, the parent beam it continues, the new cumulative
// score, the token's own log probability, finished flag and length, and the re-ordered
// cache-indirection table of decode_attn.hip.
//
// Contract (tests/beam_reference.py spells out the same in float64):
//   lp[r, v] = log_softmax(logits[r])[v]; a finished row has lp = 0 at eos and -inf elsewhere;
//   total[b, k * V + v] = cum[b * K + k] + lp[b * K + k, v]; the K largest totals of a group are taken
//   in descending order, equal totals in ascending flat index k * V + v; pick j makes new beam j:
//   token = idx % V, parent = idx / V, cum' = total, logprob = lp[parent row, token],
//   finished' = finished[parent] | (token == eos), len' = len[parent] + !finished[parent]. A pick
//   whose total is -inf (only where the group has fewer than K finite totals) carries token eos,
//   logprob -inf and finished' = 1; its parent, cum' (-inf) and len' follow the same rules.
//   Table: for t < ts[r], ind'[r, t] = ind[group row parent[r], t]; ind'[r, ts[r]] = parent[r];
//   nothing above ts[r] is touched. A row whose ts is outside [0, max_seq) leaves its table row alone.
//
// Two launches; the kernel boundary between them is the only inter-workgroup hand-off:
//  1. beam_cand_kernel, one workgroup of 1024 threads per row: the row is staged in LDS as 16-bit
//     order-preserving keys (logit_keys.h), the K-th largest key is found with two count
//     histograms (upper 11 bits, then the lower 5 inside the boundary bin), and the row's K best
//     candidates go to a workspace in order: descending key, ascending index among equal keys, of the
//     boundary key the lowest indices. Within a row the order of totals is the order of keys, so no
//     other token of the row can be among the group's K best. A candidate carries
//     lp = (val - xmax) - logf(Z * 2^-40), Z the fixed-point normaliser sampling.hip sums from the
//     same qfix: a K = 1 step scores a token exactly as greedy search does.
//  2. beam_merge_kernel, one workgroup per group: the K * K <= 256 candidates become cum + lp in fp32,
//     each finds its rank by counting the candidates ahead of it, the first K write the six outputs
//     (cum, finished and len are read into LDS before the barrier that precedes the first store), and
//     the workgroup then re-indexes the group's table in place: one thread owns one column t, reads
//     its K entries (into LDS slots of its own) and writes its K entries.
#include "logit_keys.h"

namespace pha {
namespace beam {

using namespace lk;

constexpr int MAX_R = 16, MAX_K = 16;
constexpr int MERGE_THREADS = MAX_K * MAX_K;   // one thread per candidate of a group

typedef lk::Found<false> Found;   // the scans run on counts alone: no mass arrays in LDS

struct Smem {
  u64 wt[WAVES];
  unsigned cnt1[L1_BINS];
  unsigned cnt2[L2_BINS];
  unsigned kmax[WAVES];
  unsigned ckey[MAX_K];   // the row's candidates, first in index order
  int cidx[MAX_K];
  Found found;
  int pad_[2];
};
static_assert(sizeof(Smem) % 16 == 0, "the keys behind it are stored 16 bytes at a time");
static_assert(sizeof(Smem) + 2 * MAX_V <= 160 * 1024, "one workgroup's LDS");

// cand_lp / cand_tok: [R, MAX_K]; slot j >= (what the row has) holds (-inf, V + j)
template <typename T>
__global__ __launch_bounds__(THREADS) void beam_cand_kernel(const T* __restrict__ logits, long ld,
                                                            const unsigned char* __restrict__ finished,
                                                            float* __restrict__ cand_lp, int* __restrict__ cand_tok,
                                                            int V, int K, long eos, int vec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem& sm = *reinterpret_cast<Smem*>(smem_raw);
  unsigned short* keys = reinterpret_cast<unsigned short*>(smem_raw + sizeof(Smem));
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int row = blockIdx.x;
  float* olp = cand_lp + (size_t)row * MAX_K;
  int* otok = cand_tok + (size_t)row * MAX_K;
  if (finished[row]) {   // the whole block takes this branch or none of it does
    if (tid < K) {
      olp[tid] = tid == 0 ? 0.f : -INFINITY;
      otok[tid] = tid == 0 ? (int)eos : V + tid;
    }
    return;
  }
  const int Kr = K < V ? K : V;   // candidates the row has

  // ---- stage the row as keys, find the largest (block_max's barrier publishes the zeroes too) ------
  const unsigned short* src = reinterpret_cast<const unsigned short*>(logits + (long)row * ld);
  unsigned kmax = stage_keys(src, keys, V, vec);
  for (int b = tid; b < L1_BINS; b += THREADS) sm.cnt1[b] = 0u;
  if (tid < L2_BINS) sm.cnt2[tid] = 0u;
  if (tid == 0) { sm.found.count_above = 0u; sm.found.bin = 0; }
  kmax = block_max(kmax, sm.kmax, lane, wid);
  const float xmax = val_of<T>(kmax);

  // ---- the normaliser and the first-level histogram -----------------------------------------------
  u64 zloc = 0;
  for (int i = tid; i < V; i += THREADS) {
    const unsigned k = keys[i];
    zloc += qfix<T>(k, xmax, 1.f);   // temperature 1: x * 1.f is exact
    if (Kr > 1) atomicAdd(&sm.cnt1[k >> L2_BITS], 1u);
  }
  u64 Z;
  block_scan(zloc, sm.wt, &Z);   // its barriers also publish the histogram

  // ---- the K-th key: keys above kt are candidates, and the first rt (by index) of those equal to it
  unsigned kt = kmax;
  u64 rt = 1;
  if (Kr > 1) {
    const Found f1 = scan_find<false>(sm.cnt1, nullptr, L1_BINS, false, (u64)Kr, sm.wt, &sm.found);
    for (int i = tid; i < V; i += THREADS) {
      const unsigned k = keys[i];
      if ((k >> L2_BITS) == (unsigned)f1.bin) atomicAdd(&sm.cnt2[k & (L2_BINS - 1)], 1u);
    }
    __syncthreads();
    const Found f2 = scan_find<false>(sm.cnt2, nullptr, L2_BINS, false, (u64)Kr - f1.count_above, sm.wt, &sm.found);
    kt = ((unsigned)f1.bin << L2_BITS) | (unsigned)f2.bin;
    rt = (u64)Kr - f1.count_above - f2.count_above;
  }

  // ---- collect the Kr candidates in ascending token index: thread t owns one contiguous chunk ------
  const Chunk ch = row_chunk(V);
  const int i0 = ch.i0, i1 = ch.i1;
  unsigned ties = 0u, gt = 0u;
  for (int i = i0; i < i1; ++i) {
    const unsigned k = keys[i];
    if (k > kt) ++gt;
    else if (k == kt) ++ties;
  }
  u64 tot;
  const u64 tb = block_scan((u64)ties, sm.wt, &tot);
  const u64 take = ties_taken(tb, ties, rt);
  u64 slot = block_scan((u64)gt + take, sm.wt, &tot);   // tot == Kr
  if (gt + take > 0) {
    u64 tr = tb;
    for (int i = i0; i < i1; ++i) {
      const unsigned k = keys[i];
      bool mine = k > kt;
      if (k == kt) { mine = tr < rt; ++tr; }
      if (mine && slot < (u64)MAX_K) {   // slot < Kr by construction; the bound keeps the store in the array
        sm.ckey[slot] = k;
        sm.cidx[slot] = i;
        ++slot;
      }
    }
  }
  __syncthreads();
  // descending key, ascending index among equal keys: a stable insertion sort of at most 16 entries
  if (tid == 0) {
    for (int a = 1; a < Kr; ++a) {
      const unsigned k = sm.ckey[a];
      const int ix = sm.cidx[a];
      int p = a - 1;
      while (p >= 0 && sm.ckey[p] < k) {
        sm.ckey[p + 1] = sm.ckey[p];
        sm.cidx[p + 1] = sm.cidx[p];
        --p;
      }
      sm.ckey[p + 1] = k;
      sm.cidx[p + 1] = ix;
    }
  }
  __syncthreads();
  if (tid < K) {
    float lp = -INFINITY;
    int tk = V + tid;
    if (tid < Kr) {
      const float v = val_of<T>(sm.ckey[tid]);
      const float zf = (float)Z * (1.f / FIX_ONE);
      tk = sm.cidx[tid];
      if (v != -INFINITY) lp = (v - xmax) * 1.f - logf(zf);   // a -inf logit is -inf whatever xmax is
    }
    olp[tid] = lp;
    otok[tid] = tk;
  }
}

// grid: one workgroup of MERGE_THREADS per group of K rows
__global__ __launch_bounds__(MERGE_THREADS) void beam_merge_kernel(const float* __restrict__ cand_lp,
                                                             const int* __restrict__ cand_tok, float* __restrict__ cum,
                                                             unsigned char* __restrict__ finished,
                                                             int* __restrict__ len, int64_t* __restrict__ tok,
                                                             int* __restrict__ parent, float* __restrict__ lp_out,
                                                             int* __restrict__ ind,
                                                             const int* __restrict__ ts_rows, int K, int V, long eos,
                                                             int max_seq) {
  __shared__ float s_tot[MAX_K * MAX_K], s_lp[MAX_K * MAX_K];
  __shared__ int s_tok[MAX_K * MAX_K];
  __shared__ float s_cum[MAX_K];
  __shared__ int s_len[MAX_K], s_fin[MAX_K], s_par[MAX_K], s_ts[MAX_K];
  __shared__ int s_col[MAX_K][MERGE_THREADS];
  const int tid = threadIdx.x, g = blockIdx.x, r0 = g * K;
  if (tid < K) {
    s_cum[tid] = cum[r0 + tid];
    s_len[tid] = len[r0 + tid];
    s_fin[tid] = finished[r0 + tid] ? 1 : 0;
    const int t = ts_rows[r0 + tid];
    s_ts[tid] = (t >= 0 && t < max_seq) ? t : -1;   // a bad step: the row's table is left alone
  }
  __syncthreads();
  const int n = K * K;
  if (tid < n) {
    const int k = tid / K, j = tid % K;
    s_lp[tid] = cand_lp[(size_t)(r0 + k) * MAX_K + j];
    s_tot[tid] = s_cum[k] + s_lp[tid];
    s_tok[tid] = cand_tok[(size_t)(r0 + k) * MAX_K + j];
  }
  __syncthreads();
  if (tid < n) {
    // rank = candidates ahead: a larger total, or an equal one at a lower flat index (beam, token)
    const float t = s_tot[tid];
    const int k = tid / K, tk = s_tok[tid];
    int rank = 0;
    for (int c = 0; c < n; ++c) {
      const float t2 = s_tot[c];
      const int k2 = c / K, tk2 = s_tok[c];
      const bool ahead = t2 > t || (t2 == t && (k2 < k || (k2 == k && tk2 < tk)));
      rank += (c != tid && ahead) ? 1 : 0;
    }
    if (rank < K) {   // the candidate order is total, so each rank below K has exactly one owner
      const bool dead = t == -INFINITY;
      const long token = dead ? eos : (long)tk;
      const int r = r0 + rank;
      tok[r] = token;
      parent[r] = k;
      cum[r] = t;
      lp_out[r] = dead ? -INFINITY : s_lp[tid];
      finished[r] = (unsigned char)((s_fin[k] || dead || token == eos) ? 1 : 0);
      len[r] = s_len[k] + (s_fin[k] ? 0 : 1);
      s_par[rank] = k;
    }
  }
  __syncthreads();
  // re-index: ind'[r, t] = ind[r0 + parent[r], t] for t < ts[r], ind'[r, ts[r]] = parent[r]
  int tmax = -1;
  for (int k = 0; k < K; ++k) tmax = max(tmax, s_ts[k]);
  // the thread that owns column t keeps the column's K old entries in its own LDS slots (no other
  // thread touches them, so no barrier): all K are read before the first is overwritten
  for (int t = tid; t <= tmax; t += MERGE_THREADS) {
    for (int k = 0; k < K; ++k) s_col[k][tid] = ind[(size_t)(r0 + k) * max_seq + t];
    for (int k = 0; k < K; ++k) {
      if (t <= s_ts[k]) ind[(size_t)(r0 + k) * max_seq + t] = t < s_ts[k] ? s_col[s_par[k]][tid] : s_par[k];
    }
  }
}

template <typename T>
static int launch(const void* logits, long ld, float* cum, unsigned char* finished, int* len, int64_t* tok, int* parent,
                  float* lp_out, int* ind, const int* ts_rows, float* cand_lp, int* cand_tok, int R, int V, int K,
                  long eos, int max_seq,
                  hipStream_t st) {
  static bool attr = false;
  size_t lds;
  int vec;
  const int e = keyed_launch(beam_cand_kernel<T>, attr, sizeof(Smem), logits, ld, V, &lds, &vec);
  if (e != (int)hipSuccess) return e;
  hipLaunchKernelGGL(beam_cand_kernel<T>, dim3(R), dim3(THREADS), lds, st, (const T*)logits, ld, finished, cand_lp,
                     cand_tok, V, K, eos, vec);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(R / K), dim3(MERGE_THREADS), 0, st, cand_lp, cand_tok, cum, finished, len,
                     tok, parent, lp_out, ind, ts_rows, K, V, eos, max_seq);
  return (int)hipGetLastError();
}

}  // namespace beam
}  // namespace pha

// rows and beams per call, and the largest vocabulary (sampling.hip's limit, for the same reason)
PHA_API int pha_beam_search_max_v() { return pha::lk::MAX_V; }
PHA_API int pha_beam_search_max_k() { return pha::beam::MAX_K; }

// logits [R, V] bf16 / fp16 with row stride ld (elements) and unit inner stride; cum [R] fp32, finished
// [R] bytes and len [R] int32 are read and replaced; tok [R] int64, parent [R] int32 and logprob [R] fp32
// (the picked token's log probability under its parent row) are written;
// ind int32 [R, max_seq] is re-ordered in place up to ts_rows [R]; cand_lp fp32 / cand_tok int32 are
// [R, 16] workspaces. 1 <= K <= 16, K <= V, R % K == 0, R <= 16, 2 <= V <= 65,536.
PHA_API int pha_beam_search_step(int dt, const void* logits, long ld, float* cum, unsigned char* finished, int* len,
                                 int64_t* tok, int* parent, float* logprob, int* ind, const int* ts_rows,
                                 float* cand_lp, int* cand_tok, int R, int V, int K, long eos, int max_seq, hipStream_t stream) {
  if (!logits || !cum || !finished || !len || !tok || !parent || !logprob || !ind || !ts_rows || !cand_lp || !cand_tok)
    return (int)hipErrorInvalidValue;
  if (R < 1 || R > pha::beam::MAX_R || V < 2 || V > pha::lk::MAX_V || ld < V || max_seq < 1)
    return (int)hipErrorInvalidValue;
  if (K < 1 || K > pha::beam::MAX_K || K > V || R % K != 0) return (int)hipErrorInvalidValue;
  if (dt == pha::kBF16)
    return pha::beam::launch<pha::bf16_t>(logits, ld, cum, finished, len, tok, parent, logprob, ind, ts_rows, cand_lp,
                                          cand_tok, R, V, K, eos, max_seq, stream);
  if (dt == pha::kF16)
    return pha::beam::launch<pha::half_t>(logits, ld, cum, finished, len, tok, parent, logprob, ind, ts_rows, cand_lp,
                                          cand_tok, R, V, K, eos, max_seq, stream);
  return (int)hipErrorInvalidValue;
}
