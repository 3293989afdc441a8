// Variable-length (packed) flash attention for gfx950, forward and backward: the tokens of n
// sequences lie back to back as q [Tq, H, D] / k, v [Tk, Hk, D] (bf16 / fp16, D = 64 or 128, GQA
// with H % Hk == 0), int32 cu_seqlens_q / cu_seqlens_k [n + 1] on the device give the boundaries,
// and attention never crosses one (Paddle's flash_attn_unpadded). `causal` is top-left aligned per
// sequence: query a of a sequence sees its keys b <= a, as in the dense kernels.
//
// Work split. The host never reads cu_seqlens (no sync, hipGraph-capturable, one captured graph
// serves every set of lengths with the same T and n). fav_prep's block 0 scans both arrays into the
// prefix of per-sequence tile counts (128-row tiles; int32 [n + 1] each, entry n = the total) in
// the workspace; since sum_i ceil(len_i / 128) <= floor(T / 128) + n, each main kernel is launched
// with that many tile slots per head, a bound the host has from T and n alone. A workgroup maps
// its slot to (sequence, tile) by a binary search of the prefix and exits when the slot is past
// the total: skewed lengths cost idle slots that return at once, not n * max_seqlen / 128 tiles.
// The scan gives each of its 256 threads a run of up to 256 sequences: n <= 65,536 (kMaxSeqs),
// refused above. The other blocks of fav_prep zero the output rows of tokens at or past cu[n].
//
// Kernels (4 waves, one 128-row tile of one sequence and head per workgroup, the row on the MFMA
// lane so softmax statistics stay in registers):
//   fav_fwd   S^T = K Q^T (32x32x16 MFMA, Q fragments in registers), online softmax in fp32 with
//             exp2 and the scale folded in, O^T += V^T P^T with P^T taken from the S^T accumulators
//             as the B operand (never through LDS);
//   fav_dq    S^T, dP^T = V dO^T, dS^T = P^T (dP^T - delta), dQ^T += K^T dS^T over the sequence's
//             key tiles up to the causal bound;
//   fav_dkdv  key on the lane, K / V fragments in registers; S = Q K^T started from -lse / scale,
//             dP = dO V^T started from -delta, dV^T += dO^T P, dK^T += Q^T dS over the sequence's
//             query tiles from the causal bound and over the H / Hk query heads of the key head.
// The streamed operand (K, V or Q, dO: 64-row tiles) goes through LDS as ONE padded row-major
// image per operand (pitch 2 D + 16 bytes), read by rows (ds_read_b128: MFMA A operand of the
// score products) and transposed (ds_read_b64_tr_b16: V^T, K^T, dO^T, Q^T); two buffers, the
// next tile's global loads are in flight in registers during the current tile, one barrier per
// tile.
//
// Memory safety. Boundaries are clamped to [0, T] (cu[i+1] <= cu[i] is an empty sequence with no
// tile; a boundary above T is T); every row index that forms an address is clamped into its own
// sequence [start, end - 1], which lies in [0, T - 1]; partial tiles mask rows and keys by the
// sequence end; stores are predicated on the row lying inside the workgroup's sequence.
// Defined results: o, dq of query tokens at or past cu_q[n] and dk, dv of key tokens at or past
// cu_k[n] are 0; a query sequence with no keys gets o = 0, lse = -inf and zero gradients. lse of
// tokens outside every sequence is not written.
//
// Build figures (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage; the same for
// bf16 and fp16, the larger of causal / non-causal; scratch 0 and no VGPR spill in every instantiation,
// 16 SGPRs of the causal fav_dkdv are kept in VGPR lanes):
//   kernel      D    VGPRs  AGPRs  LDS bytes  waves / SIMD
//   fav_fwd     64   136    32     36,864     3
//   fav_fwd     128  200    96     69,632     1
//   fav_dq      64   169    64     36,864     2
//   fav_dq      128  256    87     69,632     1
//   fav_dkdv    64   179    64     37,888     2
//   fav_dkdv    128  179    160    70,656     1
//   fav_prep    -    44     0      2,048      8
// Speed: measured by tools/bench_flash_varlen.py against the dense kernels on the padded batch with a
// key-padding mask; the times and token counts are in profiles/flash_varlen/README.md.
#include "fa_common.h"

namespace {

constexpr int kMaxSeqs = 65536;   // fav_prep: 256 threads x runs of up to 256 sequences
constexpr int BMV = 128;          // rows of a workgroup's tile (4 waves x 32 lanes)
constexpr int BNV = 64;           // rows of a streamed tile

struct VarlenArgs {
  const int* cu_q;
  const int* cu_k;
  const int* tiles_q;   // prefix of query tile counts [n + 1]
  const int* tiles_k;   // prefix of key tile counts [n + 1]
  int n, Tq, Tk, H, Hk;
  float scale;
  FaStrides fs;
};

// rows of tokens at or past cu[n] to clear: `heads` rows of 8 * d8 elements per token
struct ZeroJob {
  void* p;
  long tok;
  int head, heads, T;
  const int* cu;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// tokens [s, s + len) of sequence i; len > 0 implies s <= T - 1
__device__ __forceinline__ void seq_range(const int* cu, int i, int T, int& s, int& len) {
  s = clampi(cu[i], 0, T);
  len = max(clampi(cu[i + 1], 0, T) - s, 0);
}

// 16-bit rows of the tokens [t0, t0 + 32) that lie at or past cu[n]
__device__ __forceinline__ void zero_tail(const ZeroJob& z, int n, int t0, int d8, int tid) {
  if (!z.p || t0 >= z.T) return;
  const int end = clampi(z.cu[n], 0, z.T);
  if (t0 + 32 <= end) return;
  const int per_tok = z.heads * d8;
  for (int idx = tid; idx < 32 * per_tok; idx += 256) {
    const int tk = t0 + idx / per_tok, rem = idx % per_tok;
    if (tk >= end && tk < z.T)
      *reinterpret_cast<u32x4*>(reinterpret_cast<uint16_t*>(z.p) + (long)tk * z.tok + (long)(rem / d8) * z.head +
                                8 * (rem % d8)) = u32x4{0u, 0u, 0u, 0u};
  }
}

__global__ __launch_bounds__(256) void fav_prep(const int* __restrict__ cu_q, const int* __restrict__ cu_k, int n, int Tq,
                                                int Tk, int* __restrict__ ws, int d8, ZeroJob z0, ZeroJob z1,
                                                ZeroJob z2) {
  const int tid = threadIdx.x;
  if (blockIdx.x == 0) {
    __shared__ int part[2][256];
    const int run = (n + 255) / 256, lo = min(tid * run, n), hi = min(lo + run, n);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int* cu = a ? cu_k : cu_q;
      const int T = a ? Tk : Tq;
      int sum = 0;
      for (int i = lo; i < hi; ++i) {
        int s, len;
        seq_range(cu, i, T, s, len);
        sum += (len + BMV - 1) / BMV;
      }
      part[a][tid] = sum;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int* cu = a ? cu_k : cu_q;
      const int T = a ? Tk : Tq;
      int* P = ws + a * (n + 1);
      int acc = 0;
      for (int j = 0; j < tid; ++j) acc += part[a][j];
      for (int i = lo; i < hi; ++i) {
        int s, len;
        seq_range(cu, i, T, s, len);
        P[i] = acc;
        acc += (len + BMV - 1) / BMV;
      }
      if (tid == 255) P[n] = acc;
    }
    return;
  }
  const int t0 = (blockIdx.x - 1) * 32;
  zero_tail(z0, n, t0, d8, tid);
  zero_tail(z1, n, t0, d8, tid);
  zero_tail(z2, n, t0, d8, tid);
}

// slot -> (sequence, tile in sequence): the last i in [0, n - 1] with P[i] <= slot (empty sequences
// share their successor's entry, so the last one is the owner); false when the slot is past the total
__device__ __forceinline__ bool tile_of_slot(const int* __restrict__ P, int n, int slot, int& seq, int& tile) {
  if (slot >= P[n]) return false;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (P[mid] <= slot) lo = mid;
    else hi = mid - 1;
  }
  seq = lo;
  tile = slot - P[lo];
  return true;
}

// ---- the streamed 64-row tile: global -> registers -> padded LDS image ------------------------
template <int D> struct Img {
  static constexpr int PITCH = 2 * D + 16;     // bytes; b128 row reads of 16 rows and the 4-row
  static constexpr int BYTES = BNV * PITCH;    // transposed reads fall on distinct banks
  static constexpr int CPR = D / 8;            // 16-B chunks per row
  static constexpr int NLD = BNV * CPR / 256;  // chunks per thread
};

// rows r0 .. r0 + 63 (clamped to len - 1 >= 0) of one sequence's operand; base = its row 0
template <typename T, int D>
__device__ __forceinline__ void tile_ld(const T* __restrict__ base, long tok, int r0, int len, int tid,
                                        u32x4 (&reg)[Img<D>::NLD]) {
#pragma unroll
  for (int u = 0; u < Img<D>::NLD; ++u) {
    const int idx = tid + 256 * u, row = idx / Img<D>::CPR, c = idx % Img<D>::CPR;
    reg[u] = *reinterpret_cast<const u32x4*>(base + (long)min(r0 + row, len - 1) * tok + 8 * c);
  }
}

template <int D>
__device__ __forceinline__ void tile_st(unsigned char* img, int tid, const u32x4 (&reg)[Img<D>::NLD]) {
#pragma unroll
  for (int u = 0; u < Img<D>::NLD; ++u) {
    const int idx = tid + 256 * u, row = idx / Img<D>::CPR, c = idx % Img<D>::CPR;
    *reinterpret_cast<u32x4*>(img + row * Img<D>::PITCH + 16 * c) = reg[u];
  }
}

// A operand by rows: image row `row`, elements 16 kk + 8 h .. + 7
template <int D>
__device__ __forceinline__ u32x4 row_frag(const unsigned char* img, int row, int kk, int h) {
  return *reinterpret_cast<const u32x4*>(img + row * Img<D>::PITCH + 32 * kk + 16 * h);
}

// A operand of a transposed product: column 32 db + (lane & 31), image rows r0 + 4 h + {0..3} and
// r0 + 8 + 4 h + {0..3} (the order the packed accumulators give the B operand). Each 16-lane group
// reads 4 rows x 16 columns, lane (tq, tp) row tq columns 4 tp .. + 3, and receives one column.
template <int D>
__device__ __forceinline__ u32x4 tr_frag_p(const unsigned char* img, int troff, int r0, int db) {
  const unsigned char* p = img + troff + r0 * Img<D>::PITCH + 64 * db;
  const u32x2 lo = ds_read_tr16(p);
  const u32x2 hi = ds_read_tr16(p + 8 * Img<D>::PITCH);
  return u32x4{lo[0], lo[1], hi[0], hi[1]};
}
template <int D> __device__ __forceinline__ int tr_lane_off(int lane) {
  const int h = lane >> 5, g1 = (lane >> 4) & 1, tq = (lane & 15) >> 2, tp = lane & 3;
  return (4 * h + tq) * Img<D>::PITCH + 2 * (16 * g1 + 4 * tp);
}

// accumulator registers s8 .. s8 + 7 as the 8 k-values of a B operand
template <typename T> __device__ __forceinline__ u32x4 pack8(const f32x16& v, int s8) {
  u32x4 w;
  w[0] = MF<T>::pack(v[s8 + 0], v[s8 + 1]);
  w[1] = MF<T>::pack(v[s8 + 2], v[s8 + 3]);
  w[2] = MF<T>::pack(v[s8 + 4], v[s8 + 5]);
  w[3] = MF<T>::pack(v[s8 + 6], v[s8 + 7]);
  return w;
}

// -inf into the S^T accumulators (query on the lane) of keys past the sequence end or the diagonal
template <bool CAUSAL>
__device__ __forceinline__ void mask_st(f32x16 (&s)[2], int k0, int h, int q, int Lk) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const int base = k0 + kb * 32 + 4 * h;
    const int lim1 = CAUSAL ? q - base : 1 << 30, lim2 = Lk - base;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rb = (r & 3) + 8 * (r >> 2);
      s[kb][r] = ((rb > lim1) | (rb >= lim2)) ? -INFINITY : 0.f;
    }
  }
}

// D elements of an output row from the transposed accumulators (registers 4 gg .. + 3 of block db
// are elements 32 db + 8 gg + 4 h + {0..3})
template <typename T, int D>
__device__ __forceinline__ void store_row(T* row, const f32x16 (&acc)[D / 32], float mul, int h) {
#pragma unroll
  for (int db = 0; db < D / 32; ++db)
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
      u32x2 w;
      w[0] = MF<T>::pack(acc[db][4 * gg + 0] * mul, acc[db][4 * gg + 1] * mul);
      w[1] = MF<T>::pack(acc[db][4 * gg + 2] * mul, acc[db][4 * gg + 3] * mul);
      *reinterpret_cast<u32x2*>(row + db * 32 + 8 * gg + 4 * h) = w;
    }
}

// ============================================================================================
// forward
// ============================================================================================
template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(256) void fav_fwd(const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
                                               T* __restrict__ O, float* __restrict__ LSE, VarlenArgs a) {
  typedef typename MF<T>::frag frag;
  constexpr int IMG = Img<D>::BYTES, NLD = Img<D>::NLD, KK = D / 16, DB = D / 32;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * IMG];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, lr = lane & 31;
  int seq, tile;
  if (!tile_of_slot(a.tiles_q, a.n, blockIdx.x, seq, tile)) return;
  int qs, Lq, ks, Lk;
  seq_range(a.cu_q, seq, a.Tq, qs, Lq);
  seq_range(a.cu_k, seq, a.Tk, ks, Lk);
  const int q0 = tile * BMV;
  if (q0 >= Lq) return;
  const int head = blockIdx.y, hk = head / (a.H / a.Hk);
  const int wq0 = q0 + wid * 32, q = wq0 + lr;
  const long qtok = qs + min(q, Lq - 1);
  const T* Qr = Q + qtok * a.fs.q_tok + (long)head * a.fs.q_head;
  const T* Kb = K + (long)ks * a.fs.kv_tok + (long)hk * a.fs.kv_head;   // read only when Lk > 0
  const T* Vb = V + (long)ks * a.fs.kv_tok + (long)hk * a.fs.kv_head;
  frag qf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) qf[kk] = as_frag<frag>(*reinterpret_cast<const u32x4*>(Qr + 16 * kk + 8 * h));
  const float scale_log2 = a.scale * kLog2e;
  f32x16 o[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) o[db] = zero16();
  float m_run = -INFINITY, l_run = 0.f;
  const int kend = CAUSAL ? min(Lk, q0 + BMV) : Lk;
  const int ntile = (kend + BNV - 1) / BNV;
  const bool live = wq0 < Lq;   // a wave past the sequence end only helps to load
  const int troff = tr_lane_off<D>(lane);

  u32x4 kreg[NLD], vreg[NLD];
  if (ntile > 0) {
    tile_ld<T, D>(Kb, a.fs.kv_tok, 0, Lk, tid, kreg);
    tile_ld<T, D>(Vb, a.fs.kv_tok, 0, Lk, tid, vreg);
    tile_st<D>(smem, tid, kreg);
    tile_st<D>(smem + IMG, tid, vreg);
    __syncthreads();
  }
  for (int t = 0; t < ntile; ++t) {
    const int k0 = t * BNV, cur = t & 1;
    const bool more = t + 1 < ntile;
    if (more) {
      tile_ld<T, D>(Kb, a.fs.kv_tok, k0 + BNV, Lk, tid, kreg);
      tile_ld<T, D>(Vb, a.fs.kv_tok, k0 + BNV, Lk, tid, vreg);
    }
    const unsigned char* kl = smem + cur * 2 * IMG;
    const unsigned char* vl = kl + IMG;
    if (live && !(CAUSAL && k0 > wq0 + 31)) {
      f32x16 s[2];
      if ((k0 + BNV > Lk) || (CAUSAL && k0 + BNV - 1 > wq0)) {
        mask_st<CAUSAL>(s, k0, h, q, Lk);
      } else {
        s[0] = zero16();
        s[1] = zero16();
      }
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
          s[kb] = MF<T>::mma(as_frag<frag>(row_frag<D>(kl, 32 * kb + lr, kk, h)), qf[kk], s[kb]);
      float tmax = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[kb][r]);
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * scale_log2;
      // deferred rescale: the running maximum moves only when a tile exceeds it by 2^8
      if (!__all(tmax <= m_run + 8.f)) {
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = fexp2(m_run - ((m_new == -INFINITY) ? 0.f : m_new));
        l_run *= alpha;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
        m_run = m_new;
      }
      const float m_use = (m_run == -INFINITY) ? 0.f : m_run;
      float psum = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fexp2(fmaf(s[kb][r], scale_log2, -m_use));
          s[kb][r] = p;
          psum += p;
        }
      l_run += psum + __shfl_xor(psum, 32, 64);
#pragma unroll
      for (int kg = 0; kg < 4; ++kg) {   // 16 keys each
        const frag pw = as_frag<frag>(pack8<T>(s[kg >> 1], (kg & 1) * 8));
#pragma unroll
        for (int db = 0; db < DB; ++db)
          o[db] = MF<T>::mma(as_frag<frag>(tr_frag_p<D>(vl, troff, 16 * kg, db)), pw, o[db]);
      }
    }
    if (more) {
      tile_st<D>(smem + (cur ^ 1) * 2 * IMG, tid, kreg);
      tile_st<D>(smem + (cur ^ 1) * 2 * IMG + IMG, tid, vreg);
    }
    __syncthreads();
  }
  if (q < Lq) {
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    store_row<T, D>(O + qtok * a.fs.o_tok + (long)head * a.fs.o_head, o, inv, h);
    if (h == 0) LSE[(long)head * a.Tq + qtok] = l_run > 0.f ? (m_run + log2f(l_run)) * kLn2 : -INFINITY;
  }
}

// ============================================================================================
// dQ: the forward's geometry
// ============================================================================================
template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(256) void fav_dq(const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
                                              const T* __restrict__ dO, const float* __restrict__ LSE,
                                              const float* __restrict__ DELTA, T* __restrict__ dQ, VarlenArgs a) {
  typedef typename MF<T>::frag frag;
  constexpr int IMG = Img<D>::BYTES, NLD = Img<D>::NLD, KK = D / 16, DB = D / 32;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * IMG];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, lr = lane & 31;
  int seq, tile;
  if (!tile_of_slot(a.tiles_q, a.n, blockIdx.x, seq, tile)) return;
  int qs, Lq, ks, Lk;
  seq_range(a.cu_q, seq, a.Tq, qs, Lq);
  seq_range(a.cu_k, seq, a.Tk, ks, Lk);
  const int q0 = tile * BMV;
  if (q0 >= Lq) return;
  const int head = blockIdx.y, hk = head / (a.H / a.Hk);
  const int wq0 = q0 + wid * 32, q = wq0 + lr;
  const long qtok = qs + min(q, Lq - 1);
  const T* Qr = Q + qtok * a.fs.q_tok + (long)head * a.fs.q_head;
  const T* Gr = dO + qtok * a.fs.o_tok + (long)head * a.fs.o_head;
  const T* Kb = K + (long)ks * a.fs.kv_tok + (long)hk * a.fs.kv_head;
  const T* Vb = V + (long)ks * a.fs.kv_tok + (long)hk * a.fs.kv_head;
  frag qf[KK], gf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    qf[kk] = as_frag<frag>(*reinterpret_cast<const u32x4*>(Qr + 16 * kk + 8 * h));
    gf[kk] = as_frag<frag>(*reinterpret_cast<const u32x4*>(Gr + 16 * kk + 8 * h));
  }
  const float c2 = a.scale * kLog2e;
  const float nl = -LSE[(long)head * a.Tq + qtok] * kLog2e, del = DELTA[(long)head * a.Tq + qtok];
  f32x16 dqt[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) dqt[db] = zero16();
  const int kend = CAUSAL ? min(Lk, q0 + BMV) : Lk;
  const int ntile = (kend + BNV - 1) / BNV;
  const bool live = wq0 < Lq;
  const int troff = tr_lane_off<D>(lane);

  u32x4 kreg[NLD], vreg[NLD];
  if (ntile > 0) {
    tile_ld<T, D>(Kb, a.fs.kv_tok, 0, Lk, tid, kreg);
    tile_ld<T, D>(Vb, a.fs.kv_tok, 0, Lk, tid, vreg);
    tile_st<D>(smem, tid, kreg);
    tile_st<D>(smem + IMG, tid, vreg);
    __syncthreads();
  }
  for (int t = 0; t < ntile; ++t) {
    const int k0 = t * BNV, cur = t & 1;
    const bool more = t + 1 < ntile;
    if (more) {
      tile_ld<T, D>(Kb, a.fs.kv_tok, k0 + BNV, Lk, tid, kreg);
      tile_ld<T, D>(Vb, a.fs.kv_tok, k0 + BNV, Lk, tid, vreg);
    }
    const unsigned char* kl = smem + cur * 2 * IMG;
    const unsigned char* vl = kl + IMG;
    if (live && !(CAUSAL && k0 > wq0 + 31)) {
      f32x16 s[2], dp[2];
      dp[0] = zero16();
      dp[1] = zero16();
      if ((k0 + BNV > Lk) || (CAUSAL && k0 + BNV - 1 > wq0)) {
        mask_st<CAUSAL>(s, k0, h, q, Lk);
      } else {
        s[0] = zero16();
        s[1] = zero16();
      }
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          s[kb] = MF<T>::mma(as_frag<frag>(row_frag<D>(kl, 32 * kb + lr, kk, h)), qf[kk], s[kb]);
          dp[kb] = MF<T>::mma(as_frag<frag>(row_frag<D>(vl, 32 * kb + lr, kk, h)), gf[kk], dp[kb]);
        }
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[kb][r] = fexp2(fmaf(s[kb][r], c2, nl)) * (dp[kb][r] - del);
#pragma unroll
      for (int kg = 0; kg < 4; ++kg) {
        const frag w = as_frag<frag>(pack8<T>(s[kg >> 1], (kg & 1) * 8));
#pragma unroll
        for (int db = 0; db < DB; ++db)
          dqt[db] = MF<T>::mma(as_frag<frag>(tr_frag_p<D>(kl, troff, 16 * kg, db)), w, dqt[db]);
      }
    }
    if (more) {
      tile_st<D>(smem + (cur ^ 1) * 2 * IMG, tid, kreg);
      tile_st<D>(smem + (cur ^ 1) * 2 * IMG + IMG, tid, vreg);
    }
    __syncthreads();
  }
  if (q < Lq) store_row<T, D>(dQ + qtok * a.fs.dq_tok + (long)head * a.fs.dq_head, dqt, a.scale, h);
}

// ============================================================================================
// dK / dV: key on the lane; one stream of 64-query tiles over the G = H / Hk query heads
// ============================================================================================
template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(256) void fav_dkdv(const T* __restrict__ Q, const T* __restrict__ K,
                                                const T* __restrict__ V, const T* __restrict__ dO,
                                                const float* __restrict__ LSE, const float* __restrict__ DELTA,
                                                T* __restrict__ dK, T* __restrict__ dV, VarlenArgs a) {
  typedef typename MF<T>::frag frag;
  constexpr int IMG = Img<D>::BYTES, NLD = Img<D>::NLD, KK = D / 16, DB = D / 32;
  constexpr int BUF = 2 * IMG + 2 * BNV * 4;   // Q image, dO image, -lse / scale and -delta of the 64 rows
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, lr = lane & 31;
  int seq, tile;
  if (!tile_of_slot(a.tiles_k, a.n, blockIdx.x, seq, tile)) return;
  int qs, Lq, ks, Lk;
  seq_range(a.cu_q, seq, a.Tq, qs, Lq);
  seq_range(a.cu_k, seq, a.Tk, ks, Lk);
  const int k0 = tile * BMV;
  if (k0 >= Lk) return;
  const int hk = blockIdx.y, G = a.H / a.Hk;
  const int wk0 = k0 + wid * 32, key = wk0 + lr;
  const long ktok = ks + min(key, Lk - 1);
  const T* Kr = K + ktok * a.fs.kv_tok + (long)hk * a.fs.kv_head;
  const T* Vr = V + ktok * a.fs.kv_tok + (long)hk * a.fs.kv_head;
  frag kf[KK], vf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    kf[kk] = as_frag<frag>(*reinterpret_cast<const u32x4*>(Kr + 16 * kk + 8 * h));
    vf[kk] = as_frag<frag>(*reinterpret_cast<const u32x4*>(Vr + 16 * kk + 8 * h));
  }
  const float c2 = a.scale * kLog2e, nis = -1.f / a.scale;
  f32x16 dvt[DB], dkt[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) {
    dvt[db] = zero16();
    dkt[db] = zero16();
  }
  const int qstart = CAUSAL ? k0 : 0;   // a multiple of 64
  const int ntile = qstart < Lq ? (Lq - qstart + BNV - 1) / BNV : 0;
  const int niter = ntile * G;
  const bool live = wk0 < Lk;
  const int troff = tr_lane_off<D>(lane);

  u32x4 qreg[NLD], greg[NLD];
  float rcv = 0.f;
  auto load = [&](int it) {   // read only when Lq > 0: rows clamped into [qs, qs + Lq - 1]
    const int g = it / ntile, qt = qstart + (it - g * ntile) * BNV, head = hk * G + g;
    tile_ld<T, D>(Q + (long)qs * a.fs.q_tok + (long)head * a.fs.q_head, a.fs.q_tok, qt, Lq, tid, qreg);
    tile_ld<T, D>(dO + (long)qs * a.fs.o_tok + (long)head * a.fs.o_head, a.fs.o_tok, qt, Lq, tid, greg);
    if (tid < 2 * BNV)
      rcv = (tid < BNV ? LSE : DELTA)[(long)head * a.Tq + qs + min(qt + (tid & (BNV - 1)), Lq - 1)];
  };
  auto stage = [&](int buf) {
    unsigned char* b = smem + buf * BUF;
    tile_st<D>(b, tid, qreg);
    tile_st<D>(b + IMG, tid, greg);
    if (tid < 2 * BNV) reinterpret_cast<float*>(b + 2 * IMG)[tid] = tid < BNV ? rcv * nis : -rcv;
  };
  if (niter > 0) {
    load(0);
    stage(0);
    __syncthreads();
  }
  for (int it = 0; it < niter; ++it) {
    const int cur = it & 1;
    const int qt = qstart + (it % ntile) * BNV;
    const bool more = it + 1 < niter;
    if (more) load(it + 1);
    const unsigned char* qimg = smem + cur * BUF;
    const unsigned char* gimg = qimg + IMG;
    const float* rc = reinterpret_cast<const float*>(qimg + 2 * IMG);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int qh = qt + 32 * j;
      if (!live || qh >= Lq || (CAUSAL && wk0 > qh + 31)) continue;
      f32x16 sa, da;
#pragma unroll
      for (int m = 0; m < 4; ++m) {   // rows 32 j + 8 m + 4 h + {0..3}: registers 4 m .. 4 m + 3
        const float4 l4 = *reinterpret_cast<const float4*>(rc + 32 * j + 8 * m + 4 * h);
        const float4 d4 = *reinterpret_cast<const float4*>(rc + BNV + 32 * j + 8 * m + 4 * h);
        sa[4 * m + 0] = l4.x; sa[4 * m + 1] = l4.y; sa[4 * m + 2] = l4.z; sa[4 * m + 3] = l4.w;
        da[4 * m + 0] = d4.x; da[4 * m + 1] = d4.y; da[4 * m + 2] = d4.z; da[4 * m + 3] = d4.w;
      }
      if ((qh + 32 > Lq) || (wk0 + 32 > Lk) || (CAUSAL && wk0 + 31 > qh)) {
        // masked: the key is past its end, the query row is past its end, or key > query
        const int lim = key >= Lk ? 32 : (CAUSAL ? key - qh - 4 * h : -1);
        const int lim2 = Lq - qh - 4 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rb = (r & 3) + 8 * (r >> 2);
          sa[r] = ((rb < lim) | (rb >= lim2)) ? -INFINITY : sa[r];
        }
      }
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        sa = MF<T>::mma(as_frag<frag>(row_frag<D>(qimg, 32 * j + lr, kk, h)), kf[kk], sa);
        da = MF<T>::mma(as_frag<frag>(row_frag<D>(gimg, 32 * j + lr, kk, h)), vf[kk], da);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = fexp2(sa[r] * c2);
        sa[r] = p;
        da[r] = p * da[r];
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {   // 16 queries each
        const frag pw = as_frag<frag>(pack8<T>(sa, 8 * s2)), dw = as_frag<frag>(pack8<T>(da, 8 * s2));
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          dvt[db] = MF<T>::mma(as_frag<frag>(tr_frag_p<D>(gimg, troff, 32 * j + 16 * s2, db)), pw, dvt[db]);
          dkt[db] = MF<T>::mma(as_frag<frag>(tr_frag_p<D>(qimg, troff, 32 * j + 16 * s2, db)), dw, dkt[db]);
        }
      }
    }
    if (more) stage(cur ^ 1);
    __syncthreads();
  }
  if (key < Lk) {
    store_row<T, D>(dK + ktok * a.fs.dkv_tok + (long)hk * a.fs.dkv_head, dkt, a.scale, h);
    store_row<T, D>(dV + ktok * a.fs.dkv_tok + (long)hk * a.fs.dkv_head, dvt, 1.f, h);
  }
}

// ---- host side ----------------------------------------------------------------------------------
int tile_slots(int T, int n) { return T / BMV + n; }   // >= sum_i ceil(len_i / BMV), from T and n alone

bool aligned16(const void* p) { return p && ((size_t)p & 15) == 0; }
bool stride_ok(long tok, int head) { return tok > 0 && head > 0 && tok % 8 == 0 && head % 8 == 0; }

template <typename T, int D, bool C>
int launch_fwd_v(const void* q, const void* k, const void* v, void* o, float* lse, const VarlenArgs& a, int* ws,
                 hipStream_t st) {
  const ZeroJob zo{o, a.fs.o_tok, a.fs.o_head, a.H, a.Tq, a.cu_q}, none{nullptr, 0, 0, 0, 0, nullptr};
  hipLaunchKernelGGL(fav_prep, dim3(1 + (a.Tq + 31) / 32), dim3(256), 0, st, a.cu_q, a.cu_k, a.n, a.Tq, a.Tk, ws,
                     D / 8, zo, none, none);
  hipLaunchKernelGGL((fav_fwd<T, D, C>), dim3(tile_slots(a.Tq, a.n), a.H), dim3(256), 0, st, (const T*)q, (const T*)k,
                     (const T*)v, (T*)o, lse, a);
  return (int)hipGetLastError();
}

template <typename T, int D, bool C>
int launch_bwd_v(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                 void* dq, void* dk, void* dv, const VarlenArgs& a, int* ws, hipStream_t st) {
  const ZeroJob zq{dq, a.fs.dq_tok, a.fs.dq_head, a.H, a.Tq, a.cu_q};
  const ZeroJob zk{dk, a.fs.dkv_tok, a.fs.dkv_head, a.Hk, a.Tk, a.cu_k};
  const ZeroJob zv{dv, a.fs.dkv_tok, a.fs.dkv_head, a.Hk, a.Tk, a.cu_k};
  const int tmax = a.Tq > a.Tk ? a.Tq : a.Tk;
  hipLaunchKernelGGL(fav_prep, dim3(1 + (tmax + 31) / 32), dim3(256), 0, st, a.cu_q, a.cu_k, a.n, a.Tq, a.Tk, ws,
                     D / 8, zq, zk, zv);
  hipLaunchKernelGGL((fav_dkdv<T, D, C>), dim3(tile_slots(a.Tk, a.n), a.Hk), dim3(256), 0, st, (const T*)q, (const T*)k,
                     (const T*)v, (const T*)dout, lse, delta, (T*)dk, (T*)dv, a);
  hipLaunchKernelGGL((fav_dq<T, D, C>), dim3(tile_slots(a.Tq, a.n), a.H), dim3(256), 0, st, (const T*)q, (const T*)k,
                     (const T*)v, (const T*)dout, lse, delta, (T*)dq, a);
  return (int)hipGetLastError();
}

// what both entry points refuse
bool varlen_ok(int dt, const void* q, const void* k, const void* v, const void* cu_q, const void* cu_k, int n, int Tq,
               int Tk, int H, int Hk, int D, float scale, long q_tok, int q_head, long kv_tok, int kv_head, long o_tok,
               int o_head, const void* ws) {
  if (dt != kBF16 && dt != kF16) return false;
  if (D != 64 && D != 128) return false;
  if (n < 1 || n > kMaxSeqs || Tq < 1 || Tk < 1 || H < 1 || Hk < 1 || H % Hk || H > 65535) return false;
  if (!(scale > 0.f) || !(scale < INFINITY)) return false;   // a positive scale is folded into the running maximum
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !cu_q || !cu_k || !ws || ((size_t)ws & 3)) return false;
  return stride_ok(q_tok, q_head) && stride_ok(kv_tok, kv_head) && stride_ok(o_tok, o_head);
}

}  // namespace

// bytes of the workspace both calls take: the two tile-count prefixes, int32 [2][n + 1]; 0 for an n
// the kernels do not serve (1 <= n <= 65,536: the one-workgroup scan's 256 runs of up to 256)
PHA_API long pha_fa_varlen_workspace(int n) { return (n < 1 || n > kMaxSeqs) ? 0 : 2L * (n + 1) * 4; }

// q [Tq, H, D], k / v [Tk, Hk, D], o [Tq, H, D] with element strides (token, head); lse fp32 [H, Tq];
// cu_q / cu_k int32 [n + 1] on the device. Two launches on `stream`, no host read of the lengths.
PHA_API int pha_fa_varlen_fwd(int dt, const void* q, const void* k, const void* v, void* o, float* lse,
                              const int* cu_q, const int* cu_k, int n, int Tq, int Tk, int H, int Hk, int D,
                              float scale, int causal, long q_tok, int q_head, long kv_tok, int kv_head, long o_tok,
                              int o_head, void* workspace, hipStream_t stream) {
  if (!varlen_ok(dt, q, k, v, cu_q, cu_k, n, Tq, Tk, H, Hk, D, scale, q_tok, q_head, kv_tok, kv_head, o_tok, o_head,
                 workspace) || !aligned16(o) || !lse)
    return (int)hipErrorInvalidValue;
  VarlenArgs a{cu_q, cu_k, (const int*)workspace, (const int*)workspace + n + 1, n, Tq, Tk, H, Hk, scale, FaStrides{}};
  a.fs.q_tok = q_tok, a.fs.q_head = q_head, a.fs.kv_tok = kv_tok, a.fs.kv_head = kv_head;
  a.fs.o_tok = o_tok, a.fs.o_head = o_head;
  int* ws = (int*)workspace;
#define FAV(T, DD, C) launch_fwd_v<T, DD, C>(q, k, v, o, lse, a, ws, stream)
  if (dt == kBF16) {
    if (D == 64) return causal ? FAV(bf16_t, 64, true) : FAV(bf16_t, 64, false);
    return causal ? FAV(bf16_t, 128, true) : FAV(bf16_t, 128, false);
  }
  if (D == 64) return causal ? FAV(half_t, 64, true) : FAV(half_t, 64, false);
  return causal ? FAV(half_t, 128, true) : FAV(half_t, 128, false);
#undef FAV
}

// dout with the o strides; delta fp32 [H, Tq] = rowsum(o * dout) from pha_flash_attn_bwd_preprocess
// with B = 1, S = Tq; dq [Tq, H, D] with gq_tok / gq_head, dk / dv [Tk, Hk, D] with gkv_tok / gkv_head
// (already summed over the H / Hk query heads of a key head). Three launches on `stream`.
PHA_API int pha_fa_varlen_bwd(int dt, const void* q, const void* k, const void* v, const void* dout, const float* lse,
                              const float* delta, void* dq, void* dk, void* dv, const int* cu_q, const int* cu_k,
                              int n, int Tq, int Tk, int H, int Hk, int D, float scale, int causal, long q_tok,
                              int q_head, long kv_tok, int kv_head, long o_tok, int o_head, long gq_tok, int gq_head,
                              long gkv_tok, int gkv_head, void* workspace, hipStream_t stream) {
  if (!varlen_ok(dt, q, k, v, cu_q, cu_k, n, Tq, Tk, H, Hk, D, scale, q_tok, q_head, kv_tok, kv_head, o_tok, o_head,
                 workspace) || !aligned16(dout) || !aligned16(dq) || !aligned16(dk) || !aligned16(dv) || !lse ||
      !delta || !stride_ok(gq_tok, gq_head) || !stride_ok(gkv_tok, gkv_head))
    return (int)hipErrorInvalidValue;
  VarlenArgs a{cu_q, cu_k, (const int*)workspace, (const int*)workspace + n + 1, n, Tq, Tk, H, Hk, scale, FaStrides{}};
  a.fs.q_tok = q_tok, a.fs.q_head = q_head, a.fs.kv_tok = kv_tok, a.fs.kv_head = kv_head;
  a.fs.o_tok = o_tok, a.fs.o_head = o_head;
  a.fs.dq_tok = gq_tok, a.fs.dq_head = gq_head, a.fs.dkv_tok = gkv_tok, a.fs.dkv_head = gkv_head;
  int* ws = (int*)workspace;
#define FAV(T, DD, C) launch_bwd_v<T, DD, C>(q, k, v, dout, lse, delta, dq, dk, dv, a, ws, stream)
  if (dt == kBF16) {
    if (D == 64) return causal ? FAV(bf16_t, 64, true) : FAV(bf16_t, 64, false);
    return causal ? FAV(bf16_t, 128, true) : FAV(bf16_t, 128, false);
  }
  if (D == 64) return causal ? FAV(half_t, 64, true) : FAV(half_t, 64, false);
  return causal ? FAV(half_t, 128, true) : FAV(half_t, 128, false);
#undef FAV
}
