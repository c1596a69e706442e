// Full-catalog softmax cross-entropy over the item table, the (tokens x items) logits never written to HBM.
// No reference counterpart: the reference trains with one sampled negative per position (trainer.py:36-38); this is the
// usual SASRec-family alternative.  Semantics: tokens are the positions with targets != 0, candidates the items
// 1..n_items, s_tj = <h_t[:d_item], E[j]>, loss_t = logsumexp_j s_tj - s_t,y.
//
// The streaming passes, the small kernels around them and the launchers' preamble are those of srfrd_xent_common.h, shared
// with the sampled loss (srfrd_sxent.hip).  This file holds the candidate source they are instantiated with here (Catalog:
// 64-row chunks of the item table, copied coalesced), the __global__ kernels and the two entry points.  Logit tiles are formed
// exactly as the encoder's GEMMs form theirs (fp32 matrix cores, a k-ordered product chain).
//
//   forward   xent_count / xent_compact   token list
//             xent_fwd_kernel             (token tile, item split): online (max, sum of exp) per token, target logit
//             xent_finalize_kernel        merge of the splits in split order -> lse, token loss, per-block loss sums
//             xent_stats_kernel           the block sums in block order -> stats {sum, count}
//   backward  xent_count / xent_compact   token list
//             xent_dh_kernel              (token tile, item split): P = g (softmax - onehot) in-tile, dH partial = P E
//             xent_dh_reduce_kernel       the split partials in split order -> d_hidden
//             xent_de_kernel              (64-item chunk): every token tile in order, dE = P^T H
// No float atomics anywhere: every sum has a fixed order, so two identical calls are bitwise identical.

#include "srfrd_xent_common.h"

namespace srfrd {
namespace {

// ---- the candidate source: the item table's rows 0..n_items in 64-row chunks ------------------------------------------------
// A chunk is 64 * d_item contiguous floats: thread t copies elements t, t + 256, ... (coalesced).  The (row, column) of each
// of its slots is the same for every chunk and is computed once.  Entry q of chunk c is item 64 c + q; items 1..n_items take
// part, the target among them: its logit is captured from the tile, and the gradient subtracts the one-hot there.
struct Catalog {
  struct Side {};       // no per-entry side arrays: an entry's item is its index
  struct Cand { int item; bool ok; };   // ok: one of the items 1..n_items
  int off[kSlots];      // LDS offset of slot u, or -1 (beyond the chunk)
  float v[kSlots];

  __device__ __forceinline__ explicit Catalog(const XentArgs& a) {
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int e = u * kThreads + (int)threadIdx.x;
      const int r = e / a.d_item, c = e - r * a.d_item;
      off[u] = e < kItems * a.d_item ? r * kRS + c : -1;
    }
  }
  __device__ __forceinline__ void fetch(const XentArgs& a, int chunk) {
    const int64_t i0 = (int64_t)chunk * kItems;
    const int64_t rows = (int64_t)a.n_items + 1 - i0;
    const int n = (int)((rows < kItems ? rows : kItems) * a.d_item);
    const float* src = a.table + i0 * a.d_item;
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int e = u * kThreads + (int)threadIdx.x;
      v[u] = e < n ? src[e] : 0.f;
    }
  }
  __device__ __forceinline__ void put(lds_f* buf, Side&) const {
#pragma unroll
    for (int u = 0; u < kSlots; ++u)
      if (off[u] >= 0) buf[off[u]] = v[u];
  }

  static __device__ __forceinline__ Cand cand(const XentArgs& a, int c, int q, const Side&) { return owner(a, c * kItems + q); }
  static __device__ __forceinline__ bool whole(const XentArgs& a, int c) { return c > 0 && (c + 1) * kItems <= a.n_items + 1; }
  static __device__ __forceinline__ bool takes(const XentArgs&, Cand k, int) { return k.ok; }
  static __device__ __forceinline__ float logit(Cand, float acc) { return acc; }
  static __device__ __forceinline__ void capture(Cand k, int y, float x, float* __restrict__ tgt, int tok) {
    if (k.item == y) tgt[tok] = x;          // the one lane of the grid that scores the target
  }
  static __device__ __forceinline__ float prob(Cand k, int y, float acc, float l) {   // softmax - onehot
    return __expf(acc - l) - (k.item == y ? 1.f : 0.f);
  }

  // dE: a workgroup owns items 64 blockIdx.x + (0..63), walks every token tile and writes its table rows itself
  static __device__ __forceinline__ Cand owner(const XentArgs& a, int item) {
    return Cand{item, item >= 1 && item <= a.n_items};
  }
  static __device__ __forceinline__ int64_t table_row(const XentArgs& a, Cand k) {
    return k.item <= a.n_items ? k.item : a.n_items;
  }
  static __device__ __forceinline__ void tile_range(const XentArgs&, int n_tiles, int& tt0, int& tt1) {
    tt0 = 0;
    tt1 = n_tiles;
  }
  static __device__ __forceinline__ void store(const XentArgs& a, float* __restrict__ grad_table, int item, int col, float v) {
    if (item <= a.n_items) {
      float* o = grad_table + (int64_t)item * a.d_item + col;
      *o = a.accumulate ? *o + v : v;
    }
  }
};

template <int KS>
__global__ void __launch_bounds__(kThreads) xent_fwd_kernel(const XentArgs a, float* __restrict__ part_m,
                                                            float* __restrict__ part_s, float* __restrict__ tgt) {
  xent_fwd_body<Catalog, KS>(a, part_m, part_s, tgt);
}
template <int KS, int NC>
__global__ void __launch_bounds__(kThreads) xent_dh_kernel(const XentArgs a, const float* __restrict__ lse,
                                                           const float* __restrict__ d_loss, float* __restrict__ dh_part) {
  xent_dh_body<Catalog, KS, NC>(a, lse, d_loss, dh_part);
}
template <int KS, int NC>
__global__ void __launch_bounds__(kThreads) xent_de_kernel(const XentArgs a, const float* __restrict__ lse,
                                                           const float* __restrict__ d_loss, float* __restrict__ grad_table) {
  xent_de_body<Catalog, KS, NC>(a, lse, d_loss, grad_table);
}

}  // namespace
}  // namespace srfrd

using namespace srfrd;

extern "C" int64_t srfrd_xent_workspace_floats(const srfrd_layout* lay, int B, int L) {
  if (check_layout(lay) != 0 || B <= 0 || L <= 0) return 0;
  return xent_ws(*lay, B, L, 0).total;
}

extern "C" int srfrd_xent_fwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets, int B,
                              int L, float* token_loss, float* lse, float* stats, float* workspace, int64_t ws_floats,
                              void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  XentWs w;
  XentArgs a;
  if (int rc = xent_begin(lay, token_loss && lse && stats, table, hidden, targets, B, L, 0, token_loss, lse, nullptr, workspace,
                          ws_floats, st, w, a))
    return rc;
  const int tiles = (a.T + kTok - 1) / kTok;
  with_ks((lay->d_item + 3) / 4, [&](auto ks) {
    hipLaunchKernelGGL(xent_fwd_kernel<decltype(ks)::value>, dim3(tiles, w.S), dim3(kThreads), 0, st, a,
                       workspace + w.part_m, workspace + w.part_s, workspace + w.tgt);
  });
  hipLaunchKernelGGL(xent_finalize_kernel, dim3(w.nb_fin), dim3(kFinBlock), 0, st, a.idx, a.count, workspace + w.part_m,
                     workspace + w.part_s, workspace + w.tgt, 0, w.S, (int64_t)a.T, lse, token_loss, workspace + w.bsum);
  hipLaunchKernelGGL(xent_stats_kernel, dim3(1), dim3(256), 0, st, workspace + w.bsum, w.nb_fin, a.count, stats);
  return (int)hipGetLastError();
}

extern "C" int srfrd_xent_bwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                              const float* lse, const float* d_token_loss, int B, int L, float* d_hidden, float* grad_table,
                              int accumulate, float* workspace, int64_t ws_floats, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  XentWs w;
  XentArgs a;
  if (int rc = xent_begin(lay, lse && d_token_loss && d_hidden && grad_table, table, hidden, targets, B, L, 0, nullptr, nullptr,
                          d_hidden, workspace, ws_floats, st, w, a))
    return rc;
  a.accumulate = accumulate;
  const int tiles = (a.T + kTok - 1) / kTok;
  with_ks((lay->d_item + 3) / 4, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    hipLaunchKernelGGL((xent_dh_kernel<KS, nc_of<KS>()>), dim3(tiles, w.S), dim3(kThreads), 0, st, a, lse, d_token_loss,
                       workspace + w.dh);
    hipLaunchKernelGGL((xent_de_kernel<KS, nc_of<KS>()>), dim3(a.n_chunks), dim3(kThreads), 0, st, a, lse, d_token_loss,
                       grad_table);
  });
  hipLaunchKernelGGL(xent_dh_reduce_kernel, dim3((unsigned)(((int64_t)a.T * lay->d_item + 255) / 256)), dim3(256), 0, st, a,
                     workspace + w.dh, (const float*)nullptr, d_hidden);
  return (int)hipGetLastError();
}
