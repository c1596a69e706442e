// Pieces shared by the softmax cross-entropy kernels: srfrd_xent.hip (full catalog) and srfrd_sxent.hip (sampled, shared
// negatives).  Both work on the compacted token list (the positions with a target, in position order) with 16-token register
// tiles on v_mfma_f32_16x16x4_f32, an online (max, sum of exp) per token, and fixed-order merges of their split partials.
#pragma once

#include "srfrd_dev.h"

namespace srfrd {
namespace {

constexpr int kTok = 64;        // tokens per workgroup (4 waves x 16)
constexpr int kItems = 64;      // item rows per staged chunk
constexpr int kThreads = 256;
constexpr int kSlots = kItems * SRFRD_MAX_D / kThreads;   // staging elements per thread (16)
constexpr int kRS = SRFRD_MAX_D + 1;                      // LDS row stride of a staged chunk (odd: rows hit distinct banks)
constexpr int kCountBlock = 1024;
constexpr int kFinBlock = 256;
constexpr int kSplitTarget = 2048;                        // workgroups the split passes aim for (8 per CU of a 256-CU part)

__host__ __device__ inline int64_t a64(int64_t x) { return (x + 63) & ~63ll; }

// ---- token list -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCountBlock) xent_count_kernel(const int64_t* __restrict__ targets, int64_t T,
                                                                 int* __restrict__ cnt) {
  __shared__ int sw[kCountBlock / 64];
  const int64_t t = (int64_t)blockIdx.x * kCountBlock + threadIdx.x;
  const bool v = t < T && targets[t] != 0;
  const uint64_t m = __builtin_amdgcn_ballot_w64(v);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = __builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < kCountBlock / 64; ++i) s += sw[i];
    cnt[blockIdx.x] = s;
  }
}

// idx[k] = position of the k-th token; tgt[k] = 0 (the forward overwrites it with the target logit); count[0] = tokens.
// zero_out (forward): token_loss and lse are zeroed at every position (the finalize pass overwrites the tokens').
__global__ void __launch_bounds__(kCountBlock) xent_compact_kernel(const int64_t* __restrict__ targets, int64_t T,
                                                                   const int* __restrict__ cnt, int nb, int* __restrict__ idx,
                                                                   float* __restrict__ tgt, int* __restrict__ count,
                                                                   float* __restrict__ token_loss, float* __restrict__ lse) {
  __shared__ int sw[kCountBlock / 64];
  __shared__ int s_base;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (w == 0) {
    int s = 0;
    for (int i = lane; i < (int)blockIdx.x; i += 64) s += cnt[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) s_base = s;
    if (blockIdx.x == 0) {
      int tot = 0;
      for (int i = lane; i < nb; i += 64) tot += cnt[i];
      for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
      if (lane == 0) count[0] = tot;
    }
  }
  const int64_t t = (int64_t)blockIdx.x * kCountBlock + threadIdx.x;
  const bool v = t < T && targets[t] != 0;
  const uint64_t m = __builtin_amdgcn_ballot_w64(v);
  if (lane == 0) sw[w] = __builtin_popcountll(m);
  if (token_loss != nullptr && t < T) { token_loss[t] = 0.f; lse[t] = 0.f; }
  __syncthreads();
  if (v) {
    int pre = s_base;
    for (int i = 0; i < w; ++i) pre += sw[i];
    pre += __builtin_popcountll(m & ((1ull << lane) - 1ull));
    idx[pre] = (int)t;
    tgt[pre] = 0.f;
  }
}

// The 16 hidden rows of a wave as B fragments of the transposed logit product: hf[s] = H[tok(li)][4 s + lq] (0 beyond
// d_item or past the last token).  The same registers are the A fragments of the untransposed product.
template <int KS>
__device__ __forceinline__ void load_hidden(float (&hf)[KS], const float* __restrict__ hidden, int d_out, int di,
                                            const int* __restrict__ idx, int tok, int count, int lq) {
  const bool ok = tok < count;
  const int64_t row = ok ? (int64_t)idx[tok] * d_out : 0;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 4 * s + lq;
    hf[s] = (ok && k < di) ? hidden[row + k] : 0.f;
  }
}

// Logits of item tile t of the staged chunk against the wave's 16 tokens, transposed: register r of lane l is
// s(token li, item 16 t + 4 lq + r).  Four tiles at once (independent MFMA chains).
template <int KS>
__device__ __forceinline__ void logit_tiles_T(f32x4 (&acc)[4], const lds_f* buf, const float (&hf)[KS], int li, int lq) {
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    float ef[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) ef[t] = buf[(16 * t + li) * kRS + 4 * s + lq];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ef[t], hf[s], acc[t], 0, 0, 0);
  }
}

// online (max, sum of exp): one exponential per element
__device__ __forceinline__ void online(float& m, float& s, float x) {
  const float hi = fmaxf(m, x), lo = fminf(m, x);
  const float e = __expf(lo - hi);
  s = x > m ? fmaf(s, e, 1.f) : s + e;
  m = hi;
}
__device__ __forceinline__ void merge(float& m, float& s, float m2, float s2) {
  const float hi = fmaxf(m, m2);
  const float a = m == -INFINITY ? 0.f : s * __expf(m - hi);
  const float b = m2 == -INFINITY ? 0.f : s2 * __expf(m2 - hi);
  m = hi;
  s = a + b;
}

// d_hidden = 0 before the backward writes the token rows: a kernel, not hipMemsetAsync - inside a captured HIP graph the
// memset node left some of these floats non-zero (the fused cross-entropy train step replays these launchers from a graph)
__global__ void __launch_bounds__(256) zero_floats_kernel(float* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0.f;
}
inline int zero_floats(float* p, int64_t n, hipStream_t st) {
  int64_t grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;
  if (grid > 0) hipLaunchKernelGGL(zero_floats_kernel, dim3((unsigned)grid), dim3(256), 0, st, p, n);
  return (int)hipGetLastError();
}

__global__ void __launch_bounds__(256) xent_stats_kernel(const float* __restrict__ bsum, int nb, const int* __restrict__ count,
                                                         float* __restrict__ stats) {
  __shared__ float sw[4];
  float t = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) t += bsum[i];
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    stats[0] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
    stats[1] = (float)count[0];
  }
}

template <class F>
void with_ks(int ks, F&& f) {
  switch (ks) {
#define SRFRD_XENT_KS(k) case k: f(std::integral_constant<int, k>()); break;
    SRFRD_XENT_KS(1) SRFRD_XENT_KS(2) SRFRD_XENT_KS(3) SRFRD_XENT_KS(4) SRFRD_XENT_KS(5) SRFRD_XENT_KS(6)
    SRFRD_XENT_KS(7) SRFRD_XENT_KS(8) SRFRD_XENT_KS(9) SRFRD_XENT_KS(10) SRFRD_XENT_KS(11) SRFRD_XENT_KS(12)
    SRFRD_XENT_KS(13) SRFRD_XENT_KS(14) SRFRD_XENT_KS(15) SRFRD_XENT_KS(16)
#undef SRFRD_XENT_KS
    default: break;
  }
}

// the column tiles of the backward products follow from the k-steps: NC = ceil(d_item / 16) = ceil(KS / 4)
template <int KS> constexpr int nc_of() { return (KS + 3) / 4; }

int check_layout(const srfrd_layout* lay) {
  if (!lay || lay->n_items < 1 || lay->d_item < 1 || lay->d_out < lay->d_item) return SRFRD_E_ARG;
  if (lay->table_bf16 || lay->D > SRFRD_MAX_D) return SRFRD_E_UNSUPPORTED;
  return 0;
}

}  // namespace
}  // namespace srfrd
