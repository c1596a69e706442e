// Shared negatives of one sampled-softmax train step, drawn on the device so that a captured step graph draws fresh ones on
// every replay.  Slot j's draw is a counter hash (srfrd_rng.h) of the step's seed word state[2], the site SITE_NEG and j:
//   base = fmix32(state[2] + SITE_NEG * 0x9E3779B9),  h1 = fmix32(base ^ j),  h2 = fmix32(base ^ (j | 0x80000000))
// uniform:     id = 1 + mulhi32(h1, n_items)                     (integer-exact: no float rounding in the map)
// popularity:  Walker / Vose alias table over buckets 0..n_items-1: b = mulhi32(h1, n_items), u = (h2 >> 8) * 2^-24,
//              id = (u < alias_prob[b] ? b : alias_idx[b]) + 1
// out_log_q[j] = item_log_q[id] (the host builds it once as log(K q) in fp64), or log(K / n_items) without it.
// One thread per slot; every slot is written by exactly one thread with plain vector stores.
#include "srfrd_dev.h"
#include "srfrd_rng.h"

namespace srfrd {
namespace {

__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

__global__ void __launch_bounds__(256) shared_negatives_kernel(const uint32_t* __restrict__ state, int n_items, int K,
                                                              const float* __restrict__ alias_prob,
                                                              const int32_t* __restrict__ alias_idx,
                                                              const float* __restrict__ item_log_q, float uniform_log_q,
                                                              int64_t* __restrict__ out_ids, float* __restrict__ out_log_q) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= K) return;
  const uint32_t base = fmix32(state[2] + (uint32_t)SITE_NEG * 0x9E3779B9u);
  const uint32_t h1 = fmix32(base ^ (uint32_t)j);
  int b = (int)mulhi32(h1, (uint32_t)n_items);                  // in [0, n_items)
  if (alias_prob != nullptr) {
    const uint32_t h2 = fmix32(base ^ ((uint32_t)j | 0x80000000u));
    const float u = (float)(h2 >> 8) * 0x1p-24f;                 // exact: 24-bit integer times a power of two
    if (!(u < alias_prob[b])) b = min(max(alias_idx[b], 0), n_items - 1);   // (clamped: a bad table cannot read out of bounds)
  }
  const int id = b + 1;
  out_ids[j] = id;
  out_log_q[j] = item_log_q != nullptr ? item_log_q[id] : uniform_log_q;
}

}  // namespace
}  // namespace srfrd

using namespace srfrd;

extern "C" int srfrd_shared_negatives(const uint32_t* state, int n_items, int K, const float* alias_prob, const int32_t* alias_idx,
                                      const float* item_log_q, int64_t* out_ids, float* out_log_q, void* stream) {
  if (!state || !out_ids || !out_log_q || K <= 0 || n_items < 1) return SRFRD_E_ARG;
  if ((alias_prob != nullptr) != (alias_idx != nullptr)) return SRFRD_E_ARG;
  if (alias_prob != nullptr && item_log_q == nullptr) return SRFRD_E_ARG;     // the constant log(K / n) is the uniform q's only
  const float uniform_log_q = (float)log((double)K / (double)n_items);
  hipLaunchKernelGGL(shared_negatives_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, state, n_items,
                     K, alias_prob, alias_idx, item_log_q, uniform_log_q, out_ids, out_log_q);
  return (int)hipGetLastError();
}
