// Fused CTC loss for gfx950: softmax statistics, alpha / beta recursion and the gradient with respect to
// the unnormalised logits x [T][B][V] (fp32 / bf16 / fp16; all arithmetic fp32, in log space).
//   Reference: phi/kernels/gpu/warpctc_kernel.cu, warpctc_grad_kernel.cu (the warp-ctc library).
//
// No [T][B][V] log-probability tensor exists at any point. The forward reads the logits once, the
// backward reads them once and writes the gradient once; what passes between the three kernels is
//   stats [2][T*B]           row max m and log(sum exp(x - m)): the two parts of the log-sum-exp. They
//                            stay apart as in softmax_ce (ce_gelu_embed.hip): (x - m) - log sum loses
//                            nothing to the magnitude of the logits, x - lse would carry lse's rounding
//   ws    [2][B][T][2Lmax+1] plane 0: lp, overwritten by alpha; plane 1: lp, overwritten by beta - lp
//   nll   [B]                -log p(label | x), +inf for an infeasible sample
// over the blank-interleaved label l' = blank, y0, blank, y1, ..., blank (S = 2L + 1 positions). Lengths
// and labels are read on the device only (clamped to [0, T] / [0, Lmax]; a class outside [0, V) has
// probability 0), so neither direction waits for the host and a training step stays capturable.
//
// 1. ctc_rows_kernel: one wave per live (t, b) row, four rows per workgroup, in the wave-per-row style of
//    norm_softmax.hip. Online (max, sum) over 16-byte loads; a row whose base is not 16-byte aligned
//    (V % 8 != 0) gives its first and last few elements to single lanes. The wave then gathers
//    lp[s] = (x[l'_s] - m) - log sum at the S label positions into both planes. Rows with
//    t >= input_length[b] are not read.
// 2. ctc_chains_kernel: one workgroup per sample. The alpha chain (t ascending) and the beta chain
//    (t descending) depend on nothing but lp and take input_length steps each; a step is one LDS round
//    trip plus a three-way log-add-exp, pure latency. So the workgroup's first half runs alpha and the
//    second half runs beta in the same steps and under the same barrier: the T-step chain is paid once,
//    and the barrier costs the same for one chain as for two. LDS holds, per chain, a ping-pong of the
//    previous and the current row with two -inf cells on either side (no edge branches: s - 2 and
//    s + 2 always exist), and the "may skip" flags l'_s != blank && l'_s != l'_{s-2} of the sample (the
//    labels themselves are needed only for the flags: lp is already gathered). lp rows are loaded four
//    steps ahead into registers. The step barrier waits for LDS only: every workspace cell is written,
//    and its value used, by one thread, so nothing in global memory orders between threads, and a full
//    __syncthreads() would wait for the prefetches. (Threads at s >= S load the clamped cell S - 1,
//    which the thread at S - 1 owns, to keep the step free of branches; they discard the value, so its
//    order against the owner's store four steps later does not matter.) Positions s >= S hold -inf
//    throughout.
//    CTC_MAX_S = 1024 positions fit the ping-pong, so the longest label is CTC_MAX_L = 511
//    (pha_ctc_max_label); up to 128 positions run on one wave per chain, more on four.
//    alpha + beta - lp is formed by the gradient pass (plane 0 + plane 1) and not written back: the
//    chains would have to revisit T rows to save the gradient pass one add.
// 3. ctc_grad_kernel: persistent workgroups, one row at a time. exp(alpha + beta - lp + nll) of the row's
//    S positions is added by class into a V-float LDS accumulator with LDS float atomics; the row is
//    then streamed once, grad = gout[b] * (exp((x - m) - log sum) - acc[c]), and the S touched cells are
//    cleared again (the accumulator is zeroed in full only once per workgroup). Atomics, not per-class
//    ownership: at most S adds per row, colliding only on blank and on repeated labels, while ownership
//    needs each position to find the earlier positions of its class (S^2 compares, or a sort per
//    sample). The price is the order of those few adds: a gradient can differ in its last bit from run
//    to run. Dead rows, and with zero_infinity every row of an infeasible sample, are written as zeros
//    without being read. Without zero_infinity the live rows of an infeasible sample (nll = +inf) are
//    written as NaN, which is what torch's GPU ctc_loss backward followed by the log_softmax backward
//    gives there (exp(-inf + inf) at every class). The accumulator bounds V: CTC_MAX_V = 32768 (128 KB of the CU's 160 KB LDS).
#include "common.h"
#include <algorithm>

using namespace pha;

namespace {

constexpr int CTC_MAX_S = 1024;
constexpr int CTC_MAX_L = (CTC_MAX_S - 1) / 2;
constexpr int CTC_MAX_V = 32768;
constexpr int CTC_PF = 4;   // lp rows in flight per chain

__device__ __forceinline__ int clamp_len(long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// elements of the row at p before its first 16-byte boundary (p is element-aligned)
template <typename T>
__device__ __forceinline__ int row_head(const T* p, int V) {
  const int h = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(T));
  return h < V ? h : V;
}

__device__ __forceinline__ void online8(const float (&v)[8], float& m, float& s) {
  float vm = v[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) vm = fmaxf(vm, v[i]);
  const float nm = fmaxf(m, vm);
  if (nm == -INFINITY) return;   // only -inf so far: exp(-inf + inf) is NaN
  float acc = s * __expf(m - nm);
#pragma unroll
  for (int i = 0; i < 8; ++i) acc += __expf(v[i] - nm);
  m = nm;
  s = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void ctc_rows_kernel(const T* __restrict__ x, const int64_t* __restrict__ labels,
                                                       const int64_t* __restrict__ in_len,
                                                       const int64_t* __restrict__ lab_len, float* __restrict__ stats,
                                                       float* __restrict__ ws, int Tn, int B, int V, int Lmax, int blank) {
  const int lane = threadIdx.x & 63;
  const long rows = (long)Tn * B;
  const long r = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int t = (int)(r / B), b = (int)(r - (long)t * B);
  if (t >= clamp_len(in_len[b], Tn)) return;
  const T* xr = x + r * (long)V;
  const int head = row_head(xr, V), nvec = (V - head) / 8, rest = V - 8 * nvec;   // rest = head + tail < 16
  const T* xv = xr + head;
  float m = -INFINITY, s = 0.f;
  if (lane < rest) {
    const float v = Cvt<T>::ld(xr, lane < head ? lane : 8 * nvec + lane);
    m = v;
    s = v == -INFINITY ? 0.f : 1.f;
  }
  for (int i = lane; i < nvec; i += 128) {   // two vectors in flight per lane
    float v0[8], v1[8];
    Vec8<T>::ld(xv + 8L * i, v0);
    const bool two = i + 64 < nvec;
    if (two) Vec8<T>::ld(xv + 8L * (i + 64), v1);
    online8(v0, m, s);
    if (two) online8(v1, m, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    const float nm = fmaxf(m, om);
    s = (nm == -INFINITY) ? 0.f : s * __expf(m - nm) + os * __expf(om - nm);
    m = nm;
  }
  const float ls = logf(s);
  if (lane == 0) {
    stats[r] = m;
    stats[rows + r] = ls;
  }
  const int S = 2 * clamp_len(lab_len[b], Lmax) + 1, SP = 2 * Lmax + 1;
  float* w0 = ws + ((long)b * Tn + t) * SP;
  float* w1 = w0 + (long)B * Tn * SP;
  for (int p = lane; p < S; p += 64) {
    const long c = (p & 1) ? labels[(long)b * Lmax + (p >> 1)] : (long)blank;
    const float lp = (c >= 0 && c < V) ? (Cvt<T>::ld(xr, c) - m) - ls : -INFINITY;
    w0[p] = lp;
    w1[p] = lp;
  }
}

// the chains' step barrier: LDS traffic only (see the file header)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// lp + log(e^a + e^b + e^c) without a branch: -inf (never NaN) when all three are -inf, as the sum is then 0
__device__ __forceinline__ float step3(float lp, float a, float b, float c) {
  float m = fmaxf(a, fmaxf(b, c));
  m = m == -INFINITY ? 0.f : m;
  return lp + (m + logf(expf(a - m) + expf(b - m) + expf(c - m)));
}

// CW threads per chain, PPT positions per thread: CW * PPT >= 2 Lmax + 1
template <int CW, int PPT>
__global__ __launch_bounds__(2 * CW) void ctc_chains_kernel(const int64_t* __restrict__ labels,
                                                            const int64_t* __restrict__ in_len,
                                                            const int64_t* __restrict__ lab_len, float* ws,
                                                            float* __restrict__ nll, float* __restrict__ loss, int Tn,
                                                            int B, int Lmax, int blank, int zero_inf) {
  constexpr int SMAX = CW * PPT;
  __shared__ float row[2][2][SMAX + 4];      // [chain][ping-pong][2 + s]
  __shared__ unsigned char skip[SMAX + 4];   // [s]: position s may be entered from s - 2; 0 beyond S
  const int b = blockIdx.x;
  const int chain = threadIdx.x / CW, tid = threadIdx.x % CW;   // chain 0: alpha, 1: beta; uniform per wave
  const int Tb = clamp_len(in_len[b], Tn), L = clamp_len(lab_len[b], Lmax);
  const int S = 2 * L + 1, SP = 2 * Lmax + 1;
  for (int i = threadIdx.x; i < 4 * (SMAX + 4); i += 2 * CW) (&row[0][0][0])[i] = -INFINITY;
  for (int p = threadIdx.x; p < SMAX + 4; p += 2 * CW) {
    bool f = false;
    if ((p & 1) && p >= 3 && p < S) {
      const int64_t c = labels[(long)b * Lmax + (p >> 1)];
      f = c != blank && c != labels[(long)b * Lmax + (p >> 1) - 1];
    }
    skip[p] = f;
  }
  __syncthreads();
  if (Tb == 0) {   // no frame: only the empty label is possible
    if (threadIdx.x == 0) {
      const float v = L == 0 ? 0.f : INFINITY;
      nll[b] = v;
      loss[b] = (zero_inf && v == INFINITY) ? 0.f : v;
    }
    return;
  }
  // the step is straight-line code but for the store (clamped loads, selects): the compiler then counts
  // the loads in flight and waits for the oldest only
  float* w = ws + ((long)chain * B + b) * Tn * (long)SP;
  const int t0 = chain ? Tb - 1 : 0, dt = chain ? -1 : 1;
  float pf[CTC_PF][PPT];
#pragma unroll
  for (int j = 0; j < CTC_PF; ++j)
#pragma unroll
    for (int k = 0; k < PPT; ++k)
      pf[j][k] = w[(long)(t0 + dt * min(j, Tb - 1)) * SP + min(tid + k * CW, S - 1)];
  for (int step0 = 0; step0 < Tb; step0 += CTC_PF) {
#pragma unroll
    for (int j = 0; j < CTC_PF; ++j) {
      const int step = step0 + j;
      if (step >= Tb) break;   // uniform over the workgroup
      float* wr = w + (long)(t0 + dt * step) * SP;
      const float* prev = row[chain][(step & 1) ^ 1];
      float* cur = row[chain][step & 1];
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const int p = tid + k * CW;
        const bool live = p < S;
        const float lp = live ? pf[j][k] : -INFINITY;
        if (step + CTC_PF < Tb) pf[j][k] = wr[(long)dt * CTC_PF * SP + min(p, S - 1)];
        float v;
        if (step == 0)
          v = (chain ? p >= S - 2 : p < 2) ? lp : -INFINITY;
        else   // alpha: s, s - 1, s - 2 under skip[s]; beta: s, s + 1, s + 2 under skip[s + 2]
          v = step3(lp, prev[p + 2], prev[p + 2 - dt], skip[p + 1 - dt] ? prev[p + 2 - 2 * dt] : -INFINITY);
        cur[p + 2] = v;   // -inf beyond S
        if (live) wr[p] = chain ? (lp == -INFINITY ? -INFINITY : v - lp) : v;   // beta - lp: weight 0, not NaN, at lp = -inf
      }
      lds_barrier();
    }
  }
  if (threadIdx.x == 0) {
    const float* last = row[0][(Tb - 1) & 1];
    const float a = last[S - 1 + 2], c = last[S - 2 + 2];   // S == 1: the -inf cell left of position 0
    const float m = fmaxf(a, c);
    const float v = m == -INFINITY ? INFINITY : -(m + logf(expf(a - m) + expf(c - m)));
    nll[b] = v;
    loss[b] = (zero_inf && v == INFINITY) ? 0.f : v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ctc_grad_kernel(const T* __restrict__ x, const int64_t* __restrict__ labels,
                                                       const int64_t* __restrict__ in_len,
                                                       const int64_t* __restrict__ lab_len,
                                                       const float* __restrict__ stats, const float* __restrict__ ws,
                                                       const float* __restrict__ nll, const float* __restrict__ gout,
                                                       T* __restrict__ dx, int Tn, int B, int V, int Lmax, int blank,
                                                       int zero_inf) {
  extern __shared__ __attribute__((aligned(16))) float ctc_acc[];   // [V]
  const int tid = threadIdx.x;
  const long rows = (long)Tn * B;
  const int SP = 2 * Lmax + 1;
  for (int c = tid; c < V; c += 256) ctc_acc[c] = 0.f;
  __syncthreads();
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const int t = (int)(r / B), b = (int)(r - (long)t * B);
    const T* xr = x + r * (long)V;
    T* dr = dx + r * (long)V;
    const int head = row_head(xr, V), nvec = (V - head) / 8, rest = V - 8 * nvec;   // x and dx: 16-byte aligned bases
    const float nl = nll[b];
    const bool dead = t >= clamp_len(in_len[b], Tn);
    if (dead || nl == INFINITY) {   // uniform over the workgroup; the row is not read
      const float f = (dead || zero_inf) ? 0.f : NAN;   // NaN: see the file header
      const float z[8] = {f, f, f, f, f, f, f, f};
      if (tid < rest) Cvt<T>::st(dr, tid < head ? tid : 8 * nvec + tid, f);
      for (int i = tid; i < nvec; i += 256) Vec8<T>::st(dr + head + 8L * i, z);
      continue;
    }
    const int S = 2 * clamp_len(lab_len[b], Lmax) + 1;
    const float* w0 = ws + ((long)b * Tn + t) * SP;
    const float* w1 = w0 + (long)B * Tn * SP;
    for (int p = tid; p < S; p += 256) {
      const long c = (p & 1) ? labels[(long)b * Lmax + (p >> 1)] : (long)blank;
      if (c >= 0 && c < V) atomicAdd(&ctc_acc[c], expf(w0[p] + w1[p] + nl));
    }
    __syncthreads();
    const float m = stats[r], ls = stats[rows + r], g = gout[b];
    if (tid < rest) {
      const int c = tid < head ? tid : 8 * nvec + tid;
      Cvt<T>::st(dr, c, g * (__expf((Cvt<T>::ld(xr, c) - m) - ls) - ctc_acc[c]));
    }
    for (int i = tid; i < nvec; i += 256) {
      const int c = head + 8 * i;
      float v[8], o[8];
      Vec8<T>::ld(xr + c, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = g * (__expf((v[k] - m) - ls) - ctc_acc[c + k]);
      Vec8<T>::st(dr + c, o);
    }
    __syncthreads();
    for (int p = tid; p < S; p += 256) {
      const long c = (p & 1) ? labels[(long)b * Lmax + (p >> 1)] : (long)blank;
      if (c >= 0 && c < V) ctc_acc[c] = 0.f;
    }
    __syncthreads();
  }
}

bool ctc_args_ok(const void* x, int Tn, int B, int V, int Lmax) {
  return Tn >= 1 && B >= 1 && V >= 1 && V <= CTC_MAX_V && Lmax >= 0 && Lmax <= CTC_MAX_L && (uintptr_t)x % 16 == 0;
}

}  // namespace

PHA_API int pha_ctc_max_label() { return CTC_MAX_L; }
PHA_API int pha_ctc_max_v() { return CTC_MAX_V; }

// x [T][B][V] (dt), labels [B][Lmax], in_len / lab_len [B] (int64) -> stats [2][T*B], ws [2][B][T][2Lmax+1],
// nll [B] and loss [B] (nll, or 0 where it is +inf and zero_inf is set), all fp32
PHA_API int pha_ctc_fwd(int dt, const void* x, const int64_t* labels, const int64_t* in_len, const int64_t* lab_len,
                        float* stats, float* ws, float* nll, float* loss, int Tn, int B, int V, int Lmax, int blank,
                        int zero_inf, hipStream_t stream) {
  if (!ctc_args_ok(x, Tn, B, V, Lmax)) return (int)hipErrorInvalidValue;
  const long rows = (long)Tn * B;
  if ((rows + 3) / 4 > 0x7fffffffL) return (int)hipErrorInvalidValue;
  PHA_DISPATCH_T(dt, T, {
    hipLaunchKernelGGL(ctc_rows_kernel<T>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, (const T*)x, labels,
                       in_len, lab_len, stats, ws, Tn, B, V, Lmax, blank);
  });
  if (2 * Lmax + 1 <= 128)
    hipLaunchKernelGGL((ctc_chains_kernel<64, 2>), dim3(B), dim3(128), 0, stream, labels, in_len, lab_len, ws, nll, loss,
                       Tn, B, Lmax, blank, zero_inf);
  else
    hipLaunchKernelGGL((ctc_chains_kernel<256, 4>), dim3(B), dim3(512), 0, stream, labels, in_len, lab_len, ws, nll,
                       loss, Tn, B, Lmax, blank, zero_inf);
  return (int)hipGetLastError();
}

// dx [T][B][V] (dt, 16-byte aligned like x) = gout [B] (fp32) times d loss / d x, from what pha_ctc_fwd left
PHA_API int pha_ctc_bwd(int dt, const void* x, const int64_t* labels, const int64_t* in_len, const int64_t* lab_len,
                        const float* stats, const float* ws, const float* nll, const float* gout, void* dx, int Tn,
                        int B, int V, int Lmax, int blank, int zero_inf, hipStream_t stream) {
  if (!ctc_args_ok(x, Tn, B, V, Lmax) || (uintptr_t)dx % 16) return (int)hipErrorInvalidValue;
  static int cu_count[64] = {};   // per device, like the LDS-limit latches below
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return (int)hipErrorInvalidDevice;
  if (!cu_count[dev] &&
      (hipDeviceGetAttribute(&cu_count[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu_count[dev] <= 0))
    cu_count[dev] = 256;
  const int cus = cu_count[dev];
  const size_t lds = (size_t)V * 4;
  const long per_cu = std::min<long>(8, std::max<long>(1, 160 * 1024 / (long)lds));
  const unsigned grid = (unsigned)std::min<long>((long)Tn * B, per_cu * cus);
  PHA_DISPATCH_T(dt, T, {
    static bool attr_set[64] = {};
    bool& attr = attr_set[dev];
    if (!attr) {
      const hipError_t e = hipFuncSetAttribute((const void*)ctc_grad_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               CTC_MAX_V * 4);
      if (e != hipSuccess) return (int)e;
      attr = true;
    }
    hipLaunchKernelGGL(ctc_grad_kernel<T>, dim3(grid), dim3(256), lds, stream, (const T*)x, labels, in_len, lab_len, stats,
                       ws, nll, gout, (T*)dx, Tn, B, V, Lmax, blank, zero_inf);
  });
  return (int)hipGetLastError();
}
