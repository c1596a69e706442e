// K negatives per position for model.token_negatives_loss, drawn on the device outside the row user's history (the
// reference's random_neq, utils.py:14-19, with K slots per position instead of one).  Slot (b, t, k) is a counter hash
// (srfrd_rng.h) of the batch (seed, batch_index), the site SITE_TNEG, the optimizer's step seed word state[2] (0 without
// `state`), the row and the slot; all of it integer-exact, wrapping in uint32:
//   s0 = fmix32(seed ^ batch_index * 0x9E3779B9),  s1 = fmix32(s0 + SITE_TNEG * 0x9E3779B9 + state[2]),
//   s2 = fmix32(s1 + b),  e = fmix32(s2 ^ (t * K + k)),  try r < SRFRD_TNEG_TRIES: h1 = fmix32(e + 2r), h2 = fmix32(e + 2r + 1)
//   bucket = mulhi32(h1, n_items);  alias table: u = (h2 >> 8) * 2^-24, bucket = u < alias_prob[bucket] ? bucket : alias_idx[bucket]
//   candidate = bucket + 1, kept if it is not one of the user's training items; 32 clashes in a row leave the slot 0.
// One 256-thread workgroup per sequence.  With exclusion it first builds an open-addressing set of the user's items in
// dynamic LDS (4-byte slots, 0 = empty, linear probing, insertion by LDS compare-and-swap; capacity = the power of two
// >= 2 max(max_hist, 32), so the load stays <= 0.5).  Membership does not depend on the insertion order, so the output is
// deterministic.  Every probe loop is bounded by the capacity and every slot index is masked into it: a corrupt CSR can
// neither write outside the set nor spin.  Then thread i takes the row's slots c = i, i + 256, ... of its L K (c = t K + k:
// consecutive lanes take consecutive k, the int64 and fp32 stores coalesce).  Every output element is written exactly once,
// by a plain vector store.
#include "srfrd_dev.h"
#include "srfrd_rng.h"

namespace srfrd {
namespace {

__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// capacity of the LDS set for histories of up to max_hist items
inline int tneg_set_capacity(int max_hist) {
  const int m = max_hist > 32 ? max_hist : 32;
  int cap = 64;
  while (cap < 2 * m) cap <<= 1;
  return cap;
}

__global__ void __launch_bounds__(256) token_negatives_kernel(
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ items, int usernum, int n_items, int max_hist, int cap,
    const int64_t* __restrict__ users, const int64_t* __restrict__ targets, int L, int K, uint32_t s0_site,
    const uint32_t* __restrict__ state, const float* __restrict__ alias_prob, const int32_t* __restrict__ alias_idx,
    const float* __restrict__ item_log_q, float uniform_log_q, const float* __restrict__ user_log_keep, int exclude,
    int64_t* __restrict__ out_ids, float* __restrict__ out_log_q) {
  extern __shared__ __attribute__((aligned(16))) uint32_t tneg_set[];     // [cap] slots, then one flag word (exclusion only)
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int u = clamp_id(users[b], usernum);
  const int64_t* trow = targets + (int64_t)b * L;
  const uint32_t mask = (uint32_t)cap - 1u;

  if (exclude) {
    // a row without a live position skips the build
    if (tid == 0) tneg_set[cap] = 0u;
    __syncthreads();
    for (int t = tid; t < L; t += 256)
      if (trow[t] != 0) tneg_set[cap] = 1u;              // (every writer stores the same word)
    __syncthreads();
    if (tneg_set[cap] != 0u) {                           // workgroup-uniform
      for (int i = tid; i < cap; i += 256) tneg_set[i] = 0u;
      __syncthreads();
      const int64_t p0 = ptr[u];
      const int64_t len = ptr[u + 1] - p0;
      const int n = (int)(len < 0 ? 0 : (len > (int64_t)max_hist ? (int64_t)max_hist : len));
      for (int i = tid; i < n; i += 256) {
        const int32_t v = items[p0 + i];
        if (v <= 0 || v > n_items) continue;             // never a candidate (0 marks an empty slot)
        uint32_t h = fmix32((uint32_t)v) & mask;
        for (int probe = 0; probe < cap; ++probe) {
          const uint32_t old = atomicCAS(&tneg_set[h], 0u, (uint32_t)v);
          if (old == 0u || old == (uint32_t)v) break;
          h = (h + 1u) & mask;
        }
      }
      __syncthreads();
    }
  }

  const uint32_t s1 = fmix32(s0_site + (state != nullptr ? state[2] : 0u));
  const uint32_t s2 = fmix32(s1 + (uint32_t)b);
  const float keep = user_log_keep != nullptr ? user_log_keep[u] : 0.f;
  const int LK = L * K;
  const int64_t obase = (int64_t)b * LK;
  for (int c = tid; c < LK; c += 256) {
    const int t = c / K;
    int id = 0;
    if (trow[t] != 0) {
      const uint32_t e = fmix32(s2 ^ (uint32_t)c);
      for (int r = 0; r < SRFRD_TNEG_TRIES; ++r) {
        const uint32_t h1 = fmix32(e + 2u * (uint32_t)r);
        int bucket = (int)mulhi32(h1, (uint32_t)n_items);             // in [0, n_items)
        if (alias_prob != nullptr) {
          const uint32_t h2 = fmix32(e + 2u * (uint32_t)r + 1u);
          const float uu = (float)(h2 >> 8) * 0x1p-24f;               // exact: 24-bit integer times a power of two
          if (!(uu < alias_prob[bucket])) bucket = min(max(alias_idx[bucket], 0), n_items - 1);   // (a bad table cannot read out of bounds)
        }
        const uint32_t cand = (uint32_t)bucket + 1u;
        bool clash = false;
        if (exclude) {
          uint32_t h = fmix32(cand) & mask;
          for (int probe = 0; probe < cap; ++probe) {
            const uint32_t s = tneg_set[h];
            if (s == cand) { clash = true; break; }
            if (s == 0u) break;
            h = (h + 1u) & mask;
          }
        }
        if (!clash) { id = (int)cand; break; }
      }
    }
    out_ids[obase + c] = id;
    if (out_log_q != nullptr)
      out_log_q[obase + c] = id != 0 ? (item_log_q != nullptr ? item_log_q[id] : uniform_log_q) - keep : 0.f;
  }
}

}  // namespace
}  // namespace srfrd

using namespace srfrd;

extern "C" int srfrd_token_negatives(const int64_t* user_ptr, const int32_t* items, int usernum, int n_items, int max_hist,
                                     const int64_t* users, const int64_t* targets, int B, int L, int K, uint32_t seed,
                                     uint32_t batch_index, const uint32_t* state, const float* alias_prob,
                                     const int32_t* alias_idx, const float* item_log_q, const float* user_log_keep,
                                     int exclude_history, int64_t* out_ids, float* out_log_q, void* stream) {
  if (!user_ptr || !items || !users || !targets || !out_ids) return SRFRD_E_ARG;
  if (B <= 0 || L <= 0 || K <= 0 || usernum <= 0 || n_items <= 0 || max_hist < 0) return SRFRD_E_ARG;
  if ((int64_t)B * L * (1 + (int64_t)K) >= (1ll << 31)) return SRFRD_E_ARG;
  if ((alias_prob != nullptr) != (alias_idx != nullptr)) return SRFRD_E_ARG;
  if (alias_prob != nullptr && item_log_q == nullptr) return SRFRD_E_ARG;     // the constant log(K / n) is the uniform q's only
  if (exclude_history && max_hist > SRFRD_TNEG_MAX_HIST) return SRFRD_E_UNSUPPORTED;
  const int cap = tneg_set_capacity(max_hist > SRFRD_TNEG_MAX_HIST ? SRFRD_TNEG_MAX_HIST : max_hist);
  const int64_t lds = exclude_history ? ((int64_t)cap + 4) * 4 : 0;           // the set and its flag word, 16-byte granular
  if (lds > 48 * 1024) {
    const int rc = lds_opt_in((const void*)token_negatives_kernel, lds);
    if (rc != 0) return rc;
  }
  const uint32_t s0 = fmix32(seed ^ (batch_index * 0x9E3779B9u));
  const uint32_t s0_site = s0 + (uint32_t)SITE_TNEG * 0x9E3779B9u;
  const float uniform_log_q = (float)log((double)K / (double)n_items);
  hipLaunchKernelGGL(token_negatives_kernel, dim3((unsigned)B), dim3(256), (size_t)lds, (hipStream_t)stream, user_ptr, items,
                     usernum, n_items, max_hist, cap, users, targets, L, K, s0_site, state, alias_prob, alias_idx, item_log_q,
                     uniform_log_q, user_log_keep, exclude_history ? 1 : 0, out_ids, out_log_q);
  return (int)hipGetLastError();
}
