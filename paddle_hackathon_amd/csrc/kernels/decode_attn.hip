// Split-KV decode attention for cached generation (one new token per sequence).
//
// The decode stage of fused_multi_transformer attends one query row over the keys [0, ts] of a
// preallocated [2, B, H, max_seq, D] cache: a pure HBM stream of the cache. Two launches:
//
//  1. decode_attn_partial, grid (split, head, batch): split s owns the DECODE_ATTN_CHUNK key
//     positions from s * CHUNK and processes those of them that are <= ts. nsplit depends on the
//     cache shape alone, so one captured graph serves every step; a split that starts beyond ts
//     exits at once. D/8 lanes cooperate on one key (16-byte loads of K and V, four keys in
//     flight per group), every lane group runs its own online softmax in fp32, the groups are
//     merged across the wave with shuffles and across the four waves through LDS, and the
//     workgroup stores (o[D], m, l) to the workspace.
//     The split that owns position ts forms the new key and value from the raw QKV product and its
//     bias, rounds them to the storage dtype, uses the rounded registers for its own score and
//     accumulation and stores them to cache[:, b, h, ts]: no workgroup reads a row that another
//     one writes in the same launch.
//  2. decode_attn_combine, grid (head, batch): merges the ts / CHUNK + 1 live splits (it derives
//     that count from ts itself, so rows of dead splits are never read) and stores `out`.
//     The kernel boundary is the inter-workgroup hand-off.
//
// The time step is a host int or, when `ts_dev` is non-null, a device int32 read by both kernels
// (no host sync, graph-capturable). Both kernels range-check the value before any address is
// formed from it: out of range, the partial kernel touches nothing and the combine kernel fills
// `out` with NaN.
//
// Per-row form (pha_decode_attn_rows): `ts_dev` is an int32 device array [B] and batch row b uses
// ts_dev[b], so prompts of different lengths decode in one launch and every row streams only its
// own live keys. The grid is the same; each workgroup of (split, head, b) reads its row's step,
// range-checks it on its own (a bad row touches nothing and gets NaN, the others are unaffected)
// and depends on no other row. ROWS is a template parameter: the scalar instantiation is the code
// it was before.
//
// Beam-indirect form (pha_decode_attn_beam), for beam search: the B rows are groups of `beam`
// consecutive beams, and a beam's history lies scattered over its group's cache rows. `ind` int32
// [B, max_seq] names, per row and key position t < ts, the beam of the group whose cache row holds
// that key: cache row (b / beam) * beam + ind[b, t]. Nothing is moved between cache rows. Position ts
// is formed from the QKV product as above, appended to row b's own cache row and used from registers;
// ind[b, ts] is never read. An entry outside [0, beam) is checked before any address is formed from it
// and its key is left out as if masked. The rows of a group must share one step: a row reads its
// siblings' cache rows below its own ts while they append at theirs. Each workgroup stages its
// chunk's 128 table entries in LDS once (one coalesced 512-byte load and one barrier per workgroup,
// instead of a dependent 4-byte load in front of every key's 16-byte loads). BEAM is one more
// template parameter of the partial kernel; the scalar and per-row instantiations are the code they
// were before.
#include "common.h"

namespace pha {

constexpr int DECODE_ATTN_CHUNK = 128;
constexpr int DECODE_ATTN_THREADS = 256;
constexpr int DECODE_ATTN_WAVES = DECODE_ATTN_THREADS / 64;

__device__ __forceinline__ void raw_ld8(const bf16_t* p, uint4& r) { r = *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void raw_ld8(const half_t* p, uint4& r) { r = *reinterpret_cast<const uint4*>(p); }

// merge the online-softmax state (m2, l2, o2) into (m, l, o); either side may be empty (m = -inf)
__device__ __forceinline__ void osm_merge(float& m, float& l, float (&o)[8], float m2, float l2, const float (&o2)[8]) {
  const float mn = fmaxf(m, m2);
  const float a = (m == -INFINITY) ? 0.f : __expf(m - mn);
  const float b = (m2 == -INFINITY) ? 0.f : __expf(m2 - mn);
  l = l * a + l2 * b;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = o[j] * a + o2[j] * b;
  m = mn;
}

// the beam form's staged table entries; only that form instantiates it
__device__ __forceinline__ int* beam_rows() {
  __shared__ int rows[DECODE_ATTN_CHUNK];
  return rows;
}

// ws: [B, H, nsplit, D + 2] fp32 rows of (o[D], m, l)
// BEAM (with ROWS): key position t < ts of row b is read from cache row (b / beam) * beam + ind[b, t].
// Everything that names `ind`, `beam`, `srow` or `in` stands in an `if constexpr (BEAM)`: the scalar
// and per-row instantiations pass null and 1 and compile to the instructions they had before.
template <typename T, int D, bool ROWS, bool BEAM>
__global__ __launch_bounds__(DECODE_ATTN_THREADS) void decode_attn_partial(
    const T* __restrict__ qkv, const T* __restrict__ qkv_bias, T* __restrict__ cache,
    const float* __restrict__ mask, long mask_sb, long mask_sh, float scale, int ts_host,
    const int* __restrict__ ts_dev, float* __restrict__ ws, int B, int H, int max_seq, int nsplit,
    const int* __restrict__ ind, int beam) {
  constexpr int LPK = D / 8;                       // lanes per key
  constexpr int GPW = 64 / LPK;                    // lane groups per wave
  constexpr int G = DECODE_ATTN_WAVES * GPW;       // lane groups per workgroup
  constexpr int U = (G * 4 <= DECODE_ATTN_CHUNK) ? 4 : (DECODE_ATTN_CHUNK / G);   // keys in flight per group
  static_assert(U >= 1 && DECODE_ATTN_CHUNK % (G * U) == 0, "chunk must be whole passes of the workgroup");

  const int ts = ROWS ? ts_dev[blockIdx.z] : (ts_dev ? *ts_dev : ts_host);   // ROWS: ts_dev is [B]
  if (ts < 0 || ts >= max_seq) return;             // nothing is read or written with a bad time step
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int k0 = s * DECODE_ATTN_CHUNK;
  if (k0 > ts) return;                             // dead split: the combine kernel never reads its row
  const int kend = min(k0 + DECODE_ATTN_CHUNK, ts + 1);
  const bool owner = kend == ts + 1;               // this split holds position ts

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int sub = lane % LPK;                      // which 8-element slice of D
  const int grp = wid * GPW + lane / LPK;          // lane group within the workgroup

  const size_t hd = (size_t)H * D;
  const T* qrow = qkv + (size_t)b * 3 * hd + (size_t)h * D + sub * 8;
  float q[8];
  Vec8<T>::ld(qrow, q);
  if (qkv_bias) {
    float t[8];
    Vec8<T>::ld(qkv_bias + (size_t)h * D + sub * 8, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] += t[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) q[j] *= scale;

  const size_t row0 = ((size_t)b * H + h) * max_seq;                 // K rows of (b, h)
  const size_t vofs = (size_t)B * H * max_seq * D;                   // K -> V plane
  T* kbase = cache + row0 * D + sub * 8;

  float knew[8], vnew[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) knew[j] = vnew[j] = 0.f;
  if (owner) {
    Vec8<T>::ld(qrow + hd, knew);
    Vec8<T>::ld(qrow + 2 * hd, vnew);
    if (qkv_bias) {
      float t[8];
      Vec8<T>::ld(qkv_bias + hd + (size_t)h * D + sub * 8, t);
#pragma unroll
      for (int j = 0; j < 8; ++j) knew[j] += t[j];
      Vec8<T>::ld(qkv_bias + 2 * hd + (size_t)h * D + sub * 8, t);
#pragma unroll
      for (int j = 0; j < 8; ++j) vnew[j] += t[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      knew[j] = round_to<T>(knew[j]);
      vnew[j] = round_to<T>(vnew[j]);
    }
    if (tid < LPK) {                               // one lane group appends the row (exact: already rounded)
      Vec8<T>::st(kbase + (size_t)ts * D, knew);
      Vec8<T>::st(kbase + vofs + (size_t)ts * D, vnew);
    }
  }

  const float* mrow = mask ? mask + (size_t)b * mask_sb + (size_t)h * mask_sh : nullptr;

  // BEAM: the chunk's table entries are staged once, already turned into the cache row to read
  // (-1: the entry is outside [0, beam) and its key is left out). Entries at or above ts are not read.
  [[maybe_unused]] int* srow = nullptr;
  if constexpr (BEAM) {
    srow = beam_rows();
    if (tid < DECODE_ATTN_CHUNK) {
      int r = -1;
      if (k0 + tid < ts) {
        const int e = ind[(size_t)b * max_seq + k0 + tid];
        if (e >= 0 && e < beam) r = (b / beam) * beam + e;
      }
      srow[tid] = r;
    }
    __syncthreads();
  }

  float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.f;

  // U keys per lane group and pass. Measured at B=8 H=16 D=128: two passes of 4 keys beat one
  // pass of 8 (21.0 vs 25.2 us at ts = 127, 36.0 vs 38.1 us at ts = 2047; profiles/decode_attn/README.md).
  for (int it = k0; it < kend; it += G * U) {      // uniform trip count over the workgroup
    uint4 kr[U], vr[U];
    float mb[U];
    int key[U];
    [[maybe_unused]] bool in[U];                   // BEAM: false where the table entry is out of range
#pragma unroll
    for (int u = 0; u < U; ++u) {
      key[u] = it + u * G + grp;
      kr[u] = vr[u] = make_uint4(0, 0, 0, 0);
      mb[u] = 0.f;
      if constexpr (BEAM) in[u] = true;
      if (key[u] < kend) {
        if (key[u] != ts) {                        // position ts comes from registers, never from the cache
          if constexpr (BEAM) {
            const int src = srow[key[u] - k0];
            in[u] = src >= 0;
            if (in[u]) {
              const T* kb = cache + (((size_t)src * H + h) * max_seq + key[u]) * D + sub * 8;
              raw_ld8(kb, kr[u]);
              raw_ld8(kb + vofs, vr[u]);
            }
          } else {
            raw_ld8(kbase + (size_t)key[u] * D, kr[u]);
            raw_ld8(kbase + vofs + (size_t)key[u] * D, vr[u]);
          }
        }
        if (mrow) mb[u] = mrow[key[u]];
      }
    }
    float sc[U];
    float mn = m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      Vec8<T>::unpack(kr[u], kf);
      if (key[u] == ts) {
#pragma unroll
        for (int j = 0; j < 8; ++j) kf[j] = knew[j];
      }
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) d = __builtin_fmaf(q[j], kf[j], d);
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) d += __shfl_xor(d, off, 64);
      sc[u] = key[u] < kend ? d + mb[u] : -INFINITY;
      if constexpr (BEAM) {
        if (!in[u]) sc[u] = -INFINITY;
      }
      mn = fmaxf(mn, sc[u]);
    }
    const float a = (m == -INFINITY) ? 0.f : __expf(m - mn);
    l *= a;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= a;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[8];
      Vec8<T>::unpack(vr[u], vf);
      if (key[u] == ts) {
#pragma unroll
        for (int j = 0; j < 8; ++j) vf[j] = vnew[j];
      }
      const float p = (sc[u] == -INFINITY) ? 0.f : __expf(sc[u] - mn);
      l += p;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = __builtin_fmaf(p, vf[j], o[j]);
    }
    m = mn;
  }

  // lane groups of the wave
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1) {
    const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
    float o2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o2[j] = __shfl_xor(o[j], off, 64);
    osm_merge(m, l, o, m2, l2, o2);
  }
  // waves of the workgroup
  __shared__ float red[DECODE_ATTN_WAVES][D + 2];
  if (lane < LPK) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wid][sub * 8 + j] = o[j];
    if (sub == 0) { red[wid][D] = m; red[wid][D + 1] = l; }
  }
  __syncthreads();
  if (tid < LPK) {
#pragma unroll
    for (int w = 1; w < DECODE_ATTN_WAVES; ++w) {
      float o2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o2[j] = red[w][sub * 8 + j];
      osm_merge(m, l, o, red[w][D], red[w][D + 1], o2);
    }
    float* wrow = ws + (((size_t)b * H + h) * nsplit + s) * (D + 2);
#pragma unroll
    for (int j = 0; j < 8; ++j) wrow[sub * 8 + j] = o[j];
    if (sub == 0) { wrow[D] = m; wrow[D + 1] = l; }
  }
}

// one thread per element of D; out: [B, H * D]
template <typename T, bool ROWS>
__global__ void decode_attn_combine(const float* __restrict__ ws, T* __restrict__ out, int ts_host,
                                    const int* __restrict__ ts_dev, int H, int D, int max_seq, int nsplit) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const size_t bh = (size_t)b * H + h;
  const int ts = ROWS ? ts_dev[b] : (ts_dev ? *ts_dev : ts_host);
  if (ts < 0 || ts >= max_seq) {
    Cvt<T>::st(out, bh * D + d, __builtin_nanf(""));
    return;
  }
  const int nlive = ts / DECODE_ATTN_CHUNK + 1;    // <= nsplit because ts < max_seq
  const float* row = ws + bh * nsplit * (D + 2);
  float M = -INFINITY;
  for (int s = 0; s < nlive; ++s) M = fmaxf(M, row[(size_t)s * (D + 2) + D]);
  float acc = 0.f, L = 0.f;
  for (int s = 0; s < nlive; ++s) {
    const float* r = row + (size_t)s * (D + 2);
    const float ms = r[D];
    const float w = (ms == -INFINITY) ? 0.f : __expf(ms - M);
    L += w * r[D + 1];
    acc += w * r[d];
  }
  Cvt<T>::st(out, bh * D + d, L > 0.f ? acc / L : 0.f);   // every key masked out: zeros
}

// ind / beam: the beam form's table and group size; the plain forms pass null and 1
template <typename T, bool ROWS, bool BEAM>
static int decode_attn_launch(const void* qkv, const void* bias, void* cache, const float* mask, long msb, long msh,
                              float scale, int ts, const int* ts_dev, const int* ind, int beam, void* out, float* ws,
                              int B, int H, int D, int max_seq, hipStream_t st) {
  const int nsplit = (max_seq + DECODE_ATTN_CHUNK - 1) / DECODE_ATTN_CHUNK;
  const dim3 grid(nsplit, H, B);
#define PHA_DA_LAUNCH(DD)                                                                                \
  decode_attn_partial<T, DD, ROWS, BEAM><<<grid, DECODE_ATTN_THREADS, 0, st>>>(                          \
      (const T*)qkv, (const T*)bias, (T*)cache, mask, msb, msh, scale, ts, ts_dev, ws, B, H, max_seq, nsplit, \
      ind, beam)
  if (D == 32) PHA_DA_LAUNCH(32);
  else if (D == 64) PHA_DA_LAUNCH(64);
  else PHA_DA_LAUNCH(128);
#undef PHA_DA_LAUNCH
  decode_attn_combine<T, ROWS><<<dim3(H, B), D, 0, st>>>(ws, (T*)out, ts, ts_dev, H, D, max_seq, nsplit);
  return (int)hipGetLastError();
}

}  // namespace pha

PHA_API int pha_decode_attn_chunk() { return pha::DECODE_ATTN_CHUNK; }

// qkv [B, 3, H, D], qkv_bias [3, H, D] or null, cache [2, B, H, max_seq, D] (row ts written),
// mask fp32 or null with element strides (mask_sb, mask_sh) and contiguous keys, ts_dev: device
// int32 read instead of `ts` when non-null, out [B, H * D], ws fp32 [B, H, nsplit, D + 2].
PHA_API int pha_decode_attn(int dt, const void* qkv, const void* qkv_bias, void* cache, const float* mask,
                            long mask_sb, long mask_sh, float scale, int ts, const int* ts_dev, void* out, float* ws,
                            int B, int H, int D, int max_seq, hipStream_t stream) {
  if (B <= 0 || H <= 0 || max_seq <= 0 || B > 65535 || H > 65535 || (D != 32 && D != 64 && D != 128))
    return (int)hipErrorInvalidValue;
  if (!ts_dev && (ts < 0 || ts >= max_seq)) return (int)hipErrorInvalidValue;
  if (dt == pha::kBF16)
    return pha::decode_attn_launch<pha::bf16_t, false, false>(qkv, qkv_bias, cache, mask, mask_sb, mask_sh, scale, ts,
                                                              ts_dev, nullptr, 1, out, ws, B, H, D, max_seq, stream);
  if (dt == pha::kF16)
    return pha::decode_attn_launch<pha::half_t, false, false>(qkv, qkv_bias, cache, mask, mask_sb, mask_sh, scale, ts,
                                                              ts_dev, nullptr, 1, out, ws, B, H, D, max_seq, stream);
  return (int)hipErrorInvalidValue;
}

// The per-row form: as pha_decode_attn, with `ts_rows` a device int32 array [B] (never null) whose
// element b is the time step of batch row b.
PHA_API int pha_decode_attn_rows(int dt, const void* qkv, const void* qkv_bias, void* cache, const float* mask,
                                 long mask_sb, long mask_sh, float scale, const int* ts_rows, void* out, float* ws,
                                 int B, int H, int D, int max_seq, hipStream_t stream) {
  if (B <= 0 || H <= 0 || max_seq <= 0 || B > 65535 || H > 65535 || (D != 32 && D != 64 && D != 128) || !ts_rows)
    return (int)hipErrorInvalidValue;
  if (dt == pha::kBF16)
    return pha::decode_attn_launch<pha::bf16_t, true, false>(qkv, qkv_bias, cache, mask, mask_sb, mask_sh, scale, 0,
                                                             ts_rows, nullptr, 1, out, ws, B, H, D, max_seq, stream);
  if (dt == pha::kF16)
    return pha::decode_attn_launch<pha::half_t, true, false>(qkv, qkv_bias, cache, mask, mask_sb, mask_sh, scale, 0,
                                                             ts_rows, nullptr, 1, out, ws, B, H, D, max_seq, stream);
  return (int)hipErrorInvalidValue;
}

// The beam-indirect form: as pha_decode_attn_rows, with `ind` a device int32 table [B, max_seq] and
// `beam` (it divides B) the number of rows in a group. Row b reads key position t < ts_rows[b] from
// cache row (b / beam) * beam + ind[b, t] and appends position ts_rows[b] to its own cache row.
PHA_API int pha_decode_attn_beam(int dt, const void* qkv, const void* qkv_bias, void* cache, const float* mask,
                                 long mask_sb, long mask_sh, float scale, const int* ts_rows, const int* ind, int beam,
                                 void* out, float* ws, int B, int H, int D, int max_seq, hipStream_t stream) {
  if (B <= 0 || H <= 0 || max_seq <= 0 || B > 65535 || H > 65535 || (D != 32 && D != 64 && D != 128) || !ts_rows || !ind)
    return (int)hipErrorInvalidValue;
  if (beam < 1 || B % beam != 0) return (int)hipErrorInvalidValue;
  if (dt == pha::kBF16)
    return pha::decode_attn_launch<pha::bf16_t, true, true>(qkv, qkv_bias, cache, mask, mask_sb, mask_sh, scale, 0,
                                                            ts_rows, ind, beam, out, ws, B, H, D, max_seq, stream);
  if (dt == pha::kF16)
    return pha::decode_attn_launch<pha::half_t, true, true>(qkv, qkv_bias, cache, mask, mask_sb, mask_sh, scale, 0,
                                                            ts_rows, ind, beam, out, ws, B, H, D, max_seq, stream);
  return (int)hipErrorInvalidValue;
}
