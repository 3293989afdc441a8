// What the decode-attention kernels share: the split geometry, the online-softmax merge and the
// combine kernel (decode_attn.hip and decode_attn_q8.hip store the same workspace rows), and the
// int8 KV-cache quantisation rule (the decode append and the prefill store of decode_attn_q8.hip).
#pragma once
#include "common.h"

namespace pha {

constexpr int DECODE_ATTN_CHUNK = 128;
constexpr int DECODE_ATTN_THREADS = 256;
constexpr int DECODE_ATTN_WAVES = DECODE_ATTN_THREADS / 64;

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

// ---- int8 KV cache: one row x[D], already rounded to the storage dtype, spread over LPK = D / 16
// consecutive lanes with 16 elements each. Symmetric in fp32: scale = absmax / 127 (1 for a zero row),
// q = clamp(rint(x / scale), -127, 127), division correctly rounded and rint half to even, which is
// what torch's round(x / scale) gives bit for bit. Returns the lane's 16 bytes in element order; every
// lane of the group gets the row's scale.
template <int LPK>
__device__ __forceinline__ uint4 kv_q8_quantize(const float (&x)[16], float& scale) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) amax = fmaxf(amax, fabsf(x[j]));
#pragma unroll
  for (int off = 1; off < LPK; off <<= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
  scale = amax > 0.f ? amax / 127.f : 1.f;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float r = fminf(fmaxf(rintf(x[j] / scale), -127.f), 127.f);
    w[j >> 2] |= ((uint32_t)(int)r & 0xffu) << (8 * (j & 3));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// 16 int8 -> float, exactly (sign extension, then the integer conversion)
__device__ __forceinline__ void kv_q8_unpack(const uint4& r, float (&o)[16]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[4 * i] = (float)((int)(w[i] << 24) >> 24);
    o[4 * i + 1] = (float)((int)(w[i] << 16) >> 24);
    o[4 * i + 2] = (float)((int)(w[i] << 8) >> 24);
    o[4 * i + 3] = (float)((int)w[i] >> 24);
  }
}

}  // namespace pha
