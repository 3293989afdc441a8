// Split-KV decode attention over an int8 KV cache, and the prefill store that fills such a cache.
//
// The cache is int8 [2, B, H, max_seq, D] with one fp32 scale per (K or V, row, head, position) in
// scales [2, B, H, max_seq]: D + 4 bytes per row where the 16-bit cache of decode_attn.hip has 2 D.
// A row is quantised when it is appended (kv_q8_quantize, decode_attn_common.h: the row rounded to
// the dtype of qkv, scale = absmax / 127, q = rint(x / scale)); readers use float(q) * scale in fp32.
//
// decode_attn_q8_partial has the grid (split, head, batch), the chunk, the time-step and table-entry
// checks and the workspace rows (o[D], m, l) of decode_attn_partial, so decode_attn_combine finishes
// it. What differs:
//  * A 16-byte load holds 16 elements: D / 16 lanes cooperate on a key (2 / 4 / 8), each with 16 query
//    elements and 16 output accumulators in fp32. At D = 128 the 32 lane groups of the workgroup
//    cover the 128-key chunk in one pass of 4 keys in flight; at D = 64 one pass of 2; at D = 32 one
//    pass of 1 (Q8_U below; profiles/decode_attn_q8/README.md).
//  * The chunk's 128 K scales and 128 V scales go through LDS: threads 0-127 load a K scale each,
//    threads 128-255 a V scale, behind one barrier, so no dependent 4-byte load stands in front of a
//    key's 16-byte loads. In the beam form every thread derives its key's source cache row from the
//    table and loads the scale from that row; the first half also stages the row. Positions above ts,
//    and keys whose table entry is out of range, are not loaded and get the scale 0.
//  * The scale is factored out of both products: score = ks[t] * sum_j q[j] * float(k8[j]) + mask,
//    o[j] += (p * vs[t]) * float(v8[j]). The int8 elements are converted exactly (sign extension).
//  * The owner split forms the biased new key and value, rounds them to T, quantises them (every lane
//    group of the workgroup holds the same row, so every thread has both scales), and puts the packed
//    bytes and the scales where the cache's would be: position ts is scored and accumulated from
//    registers by the very arithmetic that later steps apply to the stored row. One lane group stores
//    the 16-byte pieces and one lane the two scales. No workgroup reads a row that another one writes
//    in the same launch.
//
// kv_q8_store quantises the context stage's keys and values (the biased QKV product [B, S, 3, H, D])
// into positions [0, S) with the same device function, D / 16 lanes per row. The destination's batch
// and plane strides are arguments: beam search prefills every K-th cache row through a strided view.
#include "decode_attn_common.h"

namespace pha {

// keys in flight per lane group, by D (a build may override them to measure the alternatives)
#ifndef PHA_DAQ8_U128
#define PHA_DAQ8_U128 4
#endif
#ifndef PHA_DAQ8_U64
#define PHA_DAQ8_U64 2
#endif
#ifndef PHA_DAQ8_U32
#define PHA_DAQ8_U32 1
#endif
template <int D> struct Q8_U;
template <> struct Q8_U<128> { static constexpr int v = PHA_DAQ8_U128; };
template <> struct Q8_U<64> { static constexpr int v = PHA_DAQ8_U64; };
template <> struct Q8_U<32> { static constexpr int v = PHA_DAQ8_U32; };

__device__ __forceinline__ void osm_merge16(float& m, float& l, float (&o)[16], float m2, float l2,
                                            const float (&o2)[16]) {
  const float mn = fmaxf(m, m2);
  const float a = (m == -INFINITY) ? 0.f : __expf(m - mn);
  const float b = (m2 == -INFINITY) ? 0.f : __expf(m2 - mn);
  l = l * a + l2 * b;
#pragma unroll
  for (int j = 0; j < 16; ++j) o[j] = o[j] * a + o2[j] * b;
  m = mn;
}

// 16 elements of T as floats
template <typename T>
__device__ __forceinline__ void ld16(const T* p, float (&o)[16]) {
  float a[8], b[8];
  Vec8<T>::ld(p, a);
  Vec8<T>::ld(p + 8, b);
#pragma unroll
  for (int j = 0; j < 8; ++j) { o[j] = a[j]; o[8 + j] = b[j]; }
}

// cache int8 [2, B, H, max_seq, D], scales fp32 [2, B, H, max_seq]; ws: [B, H, nsplit, D + 2] fp32
template <typename T, int D, bool ROWS, bool BEAM>
__global__ __launch_bounds__(DECODE_ATTN_THREADS) void decode_attn_q8_partial(
    const T* __restrict__ qkv, const T* __restrict__ qkv_bias, int8_t* __restrict__ cache,
    float* __restrict__ scales, const float* __restrict__ mask, long mask_sb, long mask_sh, float scale,
    int ts_host, const int* __restrict__ ts_dev, float* __restrict__ ws, int B, int H, int max_seq, int nsplit,
    const int* __restrict__ ind, int beam) {
  constexpr int LPK = D / 16;                      // lanes per key
  constexpr int GPW = 64 / LPK;                    // lane groups per wave
  constexpr int G = DECODE_ATTN_WAVES * GPW;       // lane groups per workgroup
  constexpr int U = Q8_U<D>::v;                    // keys in flight per group
  static_assert(U >= 1 && DECODE_ATTN_CHUNK % (G * U) == 0, "chunk must be whole passes of the workgroup");
  static_assert(DECODE_ATTN_THREADS == 2 * DECODE_ATTN_CHUNK, "one thread per K scale and per V scale");

  const int ts = ROWS ? ts_dev[blockIdx.z] : (ts_dev ? *ts_dev : ts_host);   // ROWS: ts_dev is [B]
  if (ts < 0 || ts >= max_seq) return;             // nothing is read or written with a bad time step
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int k0 = s * DECODE_ATTN_CHUNK;
  if (k0 > ts) return;                             // dead split: the combine kernel never reads its row
  const int kend = min(k0 + DECODE_ATTN_CHUNK, ts + 1);
  const bool owner = kend == ts + 1;               // this split holds position ts

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int sub = lane % LPK;                      // which 16-element slice of D
  const int grp = wid * GPW + lane / LPK;          // lane group within the workgroup

  const size_t hd = (size_t)H * D;
  const T* qrow = qkv + (size_t)b * 3 * hd + (size_t)h * D + sub * 16;
  float q[16];
  ld16(qrow, q);
  if (qkv_bias) {
    float t[16];
    ld16(qkv_bias + (size_t)h * D + sub * 16, t);
#pragma unroll
    for (int j = 0; j < 16; ++j) q[j] += t[j];
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) q[j] *= scale;

  const size_t row0 = ((size_t)b * H + h) * max_seq;                 // K rows of (b, h)
  const size_t sofs = (size_t)B * H * max_seq;                       // K -> V plane of the scales
  const size_t vofs = sofs * D;                                      // K -> V plane of the cache

  // the owner's new row, packed as the cache holds it, with its scales
  uint4 knew = make_uint4(0, 0, 0, 0), vnew = knew;
  float ksnew = 0.f, vsnew = 0.f;
  if (owner) {
    float kf[16], vf[16];
    ld16(qrow + hd, kf);
    ld16(qrow + 2 * hd, vf);
    if (qkv_bias) {
      float t[16];
      ld16(qkv_bias + hd + (size_t)h * D + sub * 16, t);
#pragma unroll
      for (int j = 0; j < 16; ++j) kf[j] += t[j];
      ld16(qkv_bias + 2 * hd + (size_t)h * D + sub * 16, t);
#pragma unroll
      for (int j = 0; j < 16; ++j) vf[j] += t[j];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      kf[j] = round_to<T>(kf[j]);
      vf[j] = round_to<T>(vf[j]);
    }
    knew = kv_q8_quantize<LPK>(kf, ksnew);
    vnew = kv_q8_quantize<LPK>(vf, vsnew);
    if (tid < LPK) {                               // one lane group appends the row
      int8_t* dst = cache + (row0 + ts) * D + sub * 16;
      *reinterpret_cast<uint4*>(dst) = knew;
      *reinterpret_cast<uint4*>(dst + vofs) = vnew;
    }
    if (tid == 0) {
      scales[row0 + ts] = ksnew;
      scales[sofs + row0 + ts] = vsnew;
    }
  }

  // the chunk's scales, one per thread: [0, CHUNK) of K, then of V. BEAM: with the cache row to read
  // (-1: the entry is outside [0, beam) and its key is left out). Nothing at or above ts is loaded.
  __shared__ float ssc[2 * DECODE_ATTN_CHUNK];
  [[maybe_unused]] __shared__ int srow[BEAM ? DECODE_ATTN_CHUNK : 1];
  {
    const int kk = tid & (DECODE_ATTN_CHUNK - 1), key = k0 + kk;
    const bool isv = tid >= DECODE_ATTN_CHUNK;
    float sv = 0.f;
    if (key == ts) sv = isv ? vsnew : ksnew;       // only the owner has such a key
    if constexpr (BEAM) {
      int r = key == ts ? b : -1;
      if (key < ts) {
        const int e = ind[(size_t)b * max_seq + key];
        if (e >= 0 && e < beam) {
          r = (b / beam) * beam + e;
          sv = scales[(isv ? sofs : 0) + ((size_t)r * H + h) * max_seq + key];
        }
      }
      if (!isv) srow[kk] = r;
    } else {
      if (key < ts) sv = scales[(isv ? sofs : 0) + row0 + key];
    }
    ssc[tid] = sv;
  }
  __syncthreads();

  const float* mrow = mask ? mask + (size_t)b * mask_sb + (size_t)h * mask_sh : nullptr;
  const int8_t* kbase = cache + row0 * D + sub * 16;

  float m = -INFINITY, l = 0.f, o[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) o[j] = 0.f;

  for (int it = k0; it < kend; it += G * U) {      // uniform trip count over the workgroup
    uint4 kr[U], vr[U];
    float mb[U];
    int key[U];
    bool in[U];                                    // false past kend and where the table entry is out of range
#pragma unroll
    for (int u = 0; u < U; ++u) {
      key[u] = it + u * G + grp;
      kr[u] = vr[u] = make_uint4(0, 0, 0, 0);
      mb[u] = 0.f;
      in[u] = key[u] < kend;
      if (in[u]) {
        if (key[u] == ts) {                        // position ts comes from registers, never from the cache
          kr[u] = knew;
          vr[u] = vnew;
        } else if constexpr (BEAM) {
          const int src = srow[key[u] - k0];
          in[u] = src >= 0;
          if (in[u]) {
            const int8_t* kb = cache + (((size_t)src * H + h) * max_seq + key[u]) * D + sub * 16;
            kr[u] = *reinterpret_cast<const uint4*>(kb);
            vr[u] = *reinterpret_cast<const uint4*>(kb + vofs);
          }
        } else {
          kr[u] = *reinterpret_cast<const uint4*>(kbase + (size_t)key[u] * D);
          vr[u] = *reinterpret_cast<const uint4*>(kbase + vofs + (size_t)key[u] * D);
        }
        if (mrow) mb[u] = mrow[key[u]];
      }
    }
    float sc[U];
    float mn = m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[16];
      kv_q8_unpack(kr[u], kf);
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) d = __builtin_fmaf(q[j], kf[j], d);
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) d += __shfl_xor(d, off, 64);
      sc[u] = in[u] ? ssc[(key[u] - k0) & (DECODE_ATTN_CHUNK - 1)] * d + mb[u] : -INFINITY;
      mn = fmaxf(mn, sc[u]);
    }
    const float a = (m == -INFINITY) ? 0.f : __expf(m - mn);
    l *= a;
#pragma unroll
    for (int j = 0; j < 16; ++j) o[j] *= a;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[16];
      kv_q8_unpack(vr[u], vf);
      const float p = (sc[u] == -INFINITY) ? 0.f : __expf(sc[u] - mn);
      l += p;
      const float pv = p * ssc[DECODE_ATTN_CHUNK + ((key[u] - k0) & (DECODE_ATTN_CHUNK - 1))];
#pragma unroll
      for (int j = 0; j < 16; ++j) o[j] = __builtin_fmaf(pv, vf[j], o[j]);
    }
    m = mn;
  }

  // lane groups of the wave
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1) {
    const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
    float o2[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) o2[j] = __shfl_xor(o[j], off, 64);
    osm_merge16(m, l, o, m2, l2, o2);
  }
  // waves of the workgroup
  __shared__ float red[DECODE_ATTN_WAVES][D + 2];
  if (lane < LPK) {
#pragma unroll
    for (int j = 0; j < 16; ++j) red[wid][sub * 16 + j] = o[j];
    if (sub == 0) { red[wid][D] = m; red[wid][D + 1] = l; }
  }
  __syncthreads();
  if (tid < LPK) {
#pragma unroll
    for (int w = 1; w < DECODE_ATTN_WAVES; ++w) {
      float o2[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) o2[j] = red[w][sub * 16 + j];
      osm_merge16(m, l, o, red[w][D], red[w][D + 1], o2);
    }
    float* wrow = ws + (((size_t)b * H + h) * nsplit + s) * (D + 2);
#pragma unroll
    for (int j = 0; j < 16; ++j) wrow[sub * 16 + j] = o[j];
    if (sub == 0) { wrow[D] = m; wrow[D + 1] = l; }
  }
}

// qkv [B, S, 3, H, D] (biased). Row r = ((b * S + s) * 2 + kv) * H + h goes to position s of cache row b:
// cache + kv * cache_sp + b * cache_sb (int8 elements; the scales' strides are those over D).
template <typename T, int D>
__global__ __launch_bounds__(256) void kv_q8_store(const T* __restrict__ qkv, int8_t* __restrict__ cache,
                                                   float* __restrict__ scales, long cache_sb, long cache_sp,
                                                   long nrows, int S, int H, int max_seq) {
  constexpr int LPK = D / 16;
  const int sub = threadIdx.x % LPK;
  const long r = (long)blockIdx.x * (256 / LPK) + threadIdx.x / LPK;
  const bool live = r < nrows;                     // whole lane groups are live or not
  const long rr = live ? r : 0;
  const int h = (int)(rr % H), kv = (int)(rr / H % 2);
  const long bs = rr / H / 2;
  const int s = (int)(bs % S);
  const long b = bs / S;
  float x[16];
  ld16(qkv + ((bs * 3 + 1 + kv) * H + h) * D + sub * 16, x);
  float sc;
  const uint4 p = kv_q8_quantize<LPK>(x, sc);
  if (!live) return;
  const long pos = (long)h * max_seq + s;
  *reinterpret_cast<uint4*>(cache + kv * cache_sp + b * cache_sb + pos * D + sub * 16) = p;
  if (sub == 0) scales[kv * (cache_sp / D) + b * (cache_sb / D) + pos] = sc;
}

template <typename T, bool ROWS, bool BEAM>
static int decode_attn_q8_launch(const void* qkv, const void* bias, void* cache, float* scales, const float* mask,
                                 long msb, long msh, float scale, int ts, const int* ts_dev, const int* ind, int beam,
                                 void* out, float* ws, int B, int H, int D, int max_seq, hipStream_t st) {
  const int nsplit = (max_seq + DECODE_ATTN_CHUNK - 1) / DECODE_ATTN_CHUNK;
  const dim3 grid(nsplit, H, B);
#define PHA_DAQ8_LAUNCH(DD)                                                                               \
  decode_attn_q8_partial<T, DD, ROWS, BEAM><<<grid, DECODE_ATTN_THREADS, 0, st>>>(                        \
      (const T*)qkv, (const T*)bias, (int8_t*)cache, scales, mask, msb, msh, scale, ts, ts_dev, ws, B, H, \
      max_seq, nsplit, ind, beam)
  if (D == 32) PHA_DAQ8_LAUNCH(32);
  else if (D == 64) PHA_DAQ8_LAUNCH(64);
  else PHA_DAQ8_LAUNCH(128);
#undef PHA_DAQ8_LAUNCH
  decode_attn_combine<T, ROWS><<<dim3(H, B), D, 0, st>>>(ws, (T*)out, ts, ts_dev, H, D, max_seq, nsplit);
  return (int)hipGetLastError();
}

template <typename T>
static int decode_attn_q8_forms(const void* qkv, const void* bias, void* cache, float* scales, const float* mask,
                                long msb, long msh, float scale, int ts, const int* ts_dev, int per_row, const int* ind,
                                int beam, void* out, float* ws, int B, int H, int D, int max_seq, hipStream_t st) {
  if (ind)
    return decode_attn_q8_launch<T, true, true>(qkv, bias, cache, scales, mask, msb, msh, scale, 0, ts_dev, ind, beam,
                                                out, ws, B, H, D, max_seq, st);
  if (per_row)
    return decode_attn_q8_launch<T, true, false>(qkv, bias, cache, scales, mask, msb, msh, scale, 0, ts_dev, nullptr,
                                                 1, out, ws, B, H, D, max_seq, st);
  return decode_attn_q8_launch<T, false, false>(qkv, bias, cache, scales, mask, msb, msh, scale, ts, ts_dev, nullptr, 1,
                                                out, ws, B, H, D, max_seq, st);
}

template <typename T>
static int kv_q8_store_launch(const void* qkv, void* cache, float* scales, long cache_sb, long cache_sp, int B, int S,
                              int H, int D, int max_seq, hipStream_t st) {
  const long nrows = (long)B * S * 2 * H;
  const long per = 256 / (D / 16);
  const unsigned blocks = (unsigned)((nrows + per - 1) / per);
#define PHA_KVQ8_LAUNCH(DD)                                                                                        \
  kv_q8_store<T, DD><<<blocks, 256, 0, st>>>((const T*)qkv, (int8_t*)cache, scales, cache_sb, cache_sp, nrows, S, H, \
                                             max_seq)
  if (D == 32) PHA_KVQ8_LAUNCH(32);
  else if (D == 64) PHA_KVQ8_LAUNCH(64);
  else PHA_KVQ8_LAUNCH(128);
#undef PHA_KVQ8_LAUNCH
  return (int)hipGetLastError();
}

}  // namespace pha

// As pha_decode_attn / pha_decode_attn_rows / pha_decode_attn_beam, over an int8 cache [2, B, H, max_seq, D]
// with scales fp32 [2, B, H, max_seq] (row ts of both written). The form: `ind` non-null is the
// beam-indirect one (ts_dev int32 [B], `beam` divides B); otherwise `per_row` non-zero takes ts_dev as
// int32 [B]; otherwise ts_dev, when non-null, is one device int32 read instead of `ts`.
PHA_API int pha_decode_attn_q8(int dt, const void* qkv, const void* qkv_bias, void* cache, float* scales,
                               const float* mask, long mask_sb, long mask_sh, float scale, int ts, const int* ts_dev,
                               int per_row, const int* ind, int beam, void* out, float* ws, int B, int H, int D,
                               int max_seq, hipStream_t stream) {
  if (B <= 0 || H <= 0 || max_seq <= 0 || B > 65535 || H > 65535 || (D != 32 && D != 64 && D != 128) || !scales)
    return (int)hipErrorInvalidValue;
  if ((ind || per_row) && !ts_dev) return (int)hipErrorInvalidValue;
  if (ind && (beam < 1 || B % beam != 0)) return (int)hipErrorInvalidValue;
  if (!ts_dev && (ts < 0 || ts >= max_seq)) return (int)hipErrorInvalidValue;
  if (dt == pha::kBF16)
    return pha::decode_attn_q8_forms<pha::bf16_t>(qkv, qkv_bias, cache, scales, mask, mask_sb, mask_sh, scale, ts,
                                                  ts_dev, per_row, ind, beam, out, ws, B, H, D, max_seq, stream);
  if (dt == pha::kF16)
    return pha::decode_attn_q8_forms<pha::half_t>(qkv, qkv_bias, cache, scales, mask, mask_sb, mask_sh, scale, ts,
                                                  ts_dev, per_row, ind, beam, out, ws, B, H, D, max_seq, stream);
  return (int)hipErrorInvalidValue;
}

// The prefill store: the keys and values of qkv [B, S, 3, H, D] (bf16 / fp16, biased) quantised into
// positions [0, S) of an int8 cache and its scales. cache_sb / cache_sp: the cache's batch-row and K -> V
// plane strides in int8 elements, both multiples of D (a strided row view has a larger cache_sb).
PHA_API int pha_kv_q8_store(int dt, const void* qkv, void* cache, float* scales, long cache_sb, long cache_sp, int B,
                            int S, int H, int D, int max_seq, hipStream_t stream) {
  if (B <= 0 || S <= 0 || H <= 0 || S > max_seq || (D != 32 && D != 64 && D != 128) || !cache || !scales)
    return (int)hipErrorInvalidValue;
  if (cache_sb < (long)H * max_seq * D || cache_sb % D || cache_sp % D || cache_sp < 0)
    return (int)hipErrorInvalidValue;
  if (dt == pha::kBF16)
    return pha::kv_q8_store_launch<pha::bf16_t>(qkv, cache, scales, cache_sb, cache_sp, B, S, H, D, max_seq, stream);
  if (dt == pha::kF16)
    return pha::kv_q8_store_launch<pha::half_t>(qkv, cache, scales, cache_sb, cache_sp, B, S, H, D, max_seq, stream);
  return (int)hipErrorInvalidValue;
}
