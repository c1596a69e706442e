// Merge of sorted top-k lists (include/srfrd_hip_merge.h).  Included by srfrd_rank.hip behind srfrd_rank_filter.h: the keys, the
// network and the writer are srfrd_rank_wide.h's (wide_key, wide_sort's compare-exchange, wide_write).
//
// A user's n_lists lists of list_len slots are loaded as S2 = pow2ceil(n_lists) runs of R = pow2ceil(list_len) keys, the
// odd-numbered runs reversed: sorted lists then are the state wide_sort's network reaches after its stage k = R - runs ascending
// and descending in turn - and the stages k = 2 R .. P finish the sort (8 x 1024: 36 compare-exchange steps of 91).  Every
// thread tests its key against the next one of the list while it loads; one list out of order sends the workgroup through the
// whole network instead, which sorts any arrangement of the keys - the reversal included.
#pragma once

#include "../../include/srfrd_hip_merge.h"

namespace srfrd {

// wide_sort from its stage k0 on (a sibling, not a parameter of wide_sort: a start stage there, even a constant 2, costs
// wide_select_kernel two scalar registers): k0 = 2 is the whole network; k0 = 2 R expects runs of R keys, ascending and
// descending in turn
__device__ __forceinline__ void wide_sort_tail(unsigned long long* sk, int P, int k0) {
  const int tid = threadIdx.x;
  for (int k = k0; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += kWideBlock) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long x = sk[i], y = sk[ixj];
          if ((x > y) == ((i & k) == 0)) { sk[i] = y; sk[ixj] = x; }
        }
      }
      __syncthreads();
    }
}

__global__ void __launch_bounds__(kWideBlock) wide_merge_kernel(const int64_t* __restrict__ cand_idx, const float* __restrict__ cand_val,
                                                                int n_lists, int list_len, int64_t user_stride, int64_t list_stride,
                                                                int rshift, int P, int k, int64_t* __restrict__ topk_idx,
                                                                float* __restrict__ topk_val, int32_t* __restrict__ path) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_unsorted;
  unsigned long long* sk = (unsigned long long*)smem;
  const int b = blockIdx.x, tid = threadIdx.x, R = 1 << rshift;
  const auto load = [&](int i) {
    const int run = i >> rshift, pos = i & (R - 1);
    if (run >= n_lists || pos >= list_len) return kWideEmpty;
    const int64_t at = (int64_t)b * user_stride + (int64_t)run * list_stride + pos;
    const int64_t id = cand_idx[at];
    return id < 0 ? kWideEmpty : wide_key(cand_val[at], (int)id);
  };
  if (tid == 0) s_unsorted = 0;
  __syncthreads();
  bool unsorted = false;
  for (int i = tid; i < P; i += kWideBlock) {
    const unsigned long long key = load(i);
    unsigned long long next = __shfl_down(key, 1, 64);             // key i + 1 is the next lane's, or the next wave's first
    if (((i + 1) & (R - 1)) != 0) {                                // (a run's last key has no successor; i + 1 < P otherwise)
      if ((tid & 63) == 63) next = load(i + 1);
      unsorted |= key > next;
    }
    sk[((i >> rshift) & 1) ? i ^ (R - 1) : i] = key;
  }
  if (unsorted) s_unsorted = 1;
  __syncthreads();
  const int full = s_unsorted;
  wide_sort_tail(sk, P, full ? 2 : 2 * R);
  wide_write(sk, P, b, k, topk_idx, topk_val);
  if (path && tid == 0) path[b] = full;
}

static int64_t merge_pow2ceil(int n) {
  int64_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace srfrd

extern "C" int64_t srfrd_topk_merge_runs_lds_bytes(int n_lists, int list_len) {
  if (n_lists < 1 || list_len < 1) return 0;
  const int64_t P = merge_pow2ceil(n_lists) * merge_pow2ceil(list_len);
  return P > kWideCap ? 0 : 8 * P;
}

extern "C" int srfrd_topk_merge_runs(const int64_t* cand_idx, const float* cand_val, int B, int n_lists, int list_len,
                                     int64_t user_stride, int64_t list_stride, int k, int64_t* topk_idx, float* topk_val,
                                     int32_t* path, void* stream) {
  if (!cand_idx || !cand_val || !topk_idx || !topk_val || B < 1 || n_lists < 1 || list_len < 1 || k < 1 || k > kWideMax ||
      user_stride < 1 || (n_lists > 1 && list_stride < list_len))
    return SRFRD_E_ARG;
  const int64_t lds = srfrd_topk_merge_runs_lds_bytes(n_lists, list_len);
  if (lds == 0) return SRFRD_E_UNSUPPORTED;
  int rshift = 0;
  while ((1 << rshift) < list_len) ++rshift;
  if (lds > 48 * 1024 && lds_opt_in((const void*)wide_merge_kernel, lds)) return SRFRD_E_DEVICE;
  hipLaunchKernelGGL(wide_merge_kernel, dim3(B), dim3(kWideBlock), (size_t)lds, (hipStream_t)stream, cand_idx, cand_val, n_lists,
                     list_len, user_stride, list_stride, rshift, (int)(lds / 8), k, topk_idx, topk_val, path);
  return (int)hipGetLastError();
}
