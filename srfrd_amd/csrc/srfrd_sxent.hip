// Sampled softmax cross-entropy with shared negatives: every token is scored against its own target and one set of K
// sampled items shared by the whole batch, the (tokens x (1 + K)) logits never written to HBM.  No reference counterpart
// (the reference trains with one sampled negative per position, trainer.py:36-38).  Semantics: tokens are the positions
// with targets != 0; s_t+ = <h_t[:d_item], E[y_t]>; negative slot j has s_tj = <h_t[:d_item], E[n_j]> - log_q[j] (nothing
// subtracted without log_q); loss_t = logsumexp({s_t+} u {s_tj : n_j != 0, n_j != y_t if remove_hits}) - s_t+.
//
// The streaming passes, the small kernels around them and the launchers' preamble are those of srfrd_xent_common.h, shared
// with the full-catalog loss (srfrd_xent.hip).  This file holds the candidate source they are instantiated with here
// (Negatives), the __global__ kernels, the two kernels without a catalog counterpart and the two entry points.  Where xent
// streams contiguous 64-row chunks of the table, Negatives streams 64-slot chunks of the negatives, gathering the rows E[n_j]
// by id into LDS with the slot ids and log_q beside them; id-0 slots and accidental hits are masked by a compare against
// the token's target.  The target logit is one fixed-order dot product per token (sxent_target_kernel), not a tile entry.
//
//   forward   xent_count / xent_compact   token list
//             sxent_target_kernel         s_t+ per position
//             sxent_fwd_kernel            (token tile, slot split): online (max, sum of exp) per token
//             xent_finalize_kernel        (s_t+, 1) merged with the splits in split order -> lse, token loss, block sums
//             xent_stats_kernel           the block sums in block order -> stats {sum, count}
//   backward  xent_count / xent_compact   token list
//             sxent_target_kernel         g_t+ = d_t (softmax_t+ - 1), its table contribution row g_t+ h_t and key y_t
//             sxent_dh_kernel             (token tile, slot split): P = d_t softmax in-tile, dH partial = P E_neg
//             xent_dh_reduce_kernel       the split partials in split order, then g_t+ E[y_t] -> d_hidden
//             sxent_de_kernel             (64-slot chunk, token split): dE partial = P^T H over its token tiles in order
//             sxent_de_reduce_kernel      the token-split partials in split order -> one contribution row per slot, its key
// The table gradient is left as (K + B L) contribution rows with their item ids as keys, which the caller sums per item
// with srfrd_table_reduce after a stable sort.  No float atomics anywhere: two identical calls are bitwise identical.

#include "srfrd_xent_common.h"

namespace srfrd {
namespace {

constexpr int kTargetBlock = 256;

// slot j's item id (clamped; 0 for an unused slot or j >= K) and its log-Q correction (0 where it takes no part)
__device__ __forceinline__ int slot_id(const XentArgs& a, int j) { return j < a.K ? clamp_id(a.neg[j], a.n_items) : 0; }
__device__ __forceinline__ float slot_lq(const XentArgs& a, int j, int id) {
  return (a.log_q != nullptr && id != 0) ? a.log_q[j] : 0.f;
}

// ---- the candidate source: the K shared negatives in 64-slot chunks, gathered ---------------------------------------------
// Element e = u * 256 + tid of a chunk is (slot row e / d_item, column e % d_item), read from E[n_j] (zeros for unused slots
// and past K).  Threads 0..63 also fetch their slot's id and log_q into the chunk's side arrays.  A slot takes part for a
// token unless it is unused (id 0) or an accidental hit being removed; its logit is the product minus log_q.
struct Negatives {
  struct Side { int id[kItems]; float lq[kItems]; };
  struct Cand { int id; float lq; };
  int off[kSlots];      // LDS offset of element u, or -1 (beyond the chunk)
  int row[kSlots];      // its slot row in the chunk
  int col[kSlots];
  float v[kSlots];
  Cand mine;            // threads 0..63: the staged side entry

  __device__ __forceinline__ explicit Negatives(const XentArgs& a) {
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int e = u * kThreads + (int)threadIdx.x;
      const int r = e / a.d_item, c = e - r * a.d_item;
      off[u] = e < kItems * a.d_item ? r * kRS + c : -1;
      row[u] = r;
      col[u] = c;
    }
  }
  __device__ __forceinline__ void fetch(const XentArgs& a, int chunk) {
    const int j0 = chunk * kItems;
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      float x = 0.f;
      if (off[u] >= 0) {
        const int id = slot_id(a, j0 + row[u]);
        if (id != 0) x = a.table[(int64_t)id * a.d_item + col[u]];
      }
      v[u] = x;
    }
    if (threadIdx.x < kItems) mine = owner(a, j0 + (int)threadIdx.x);
  }
  __device__ __forceinline__ void put(lds_f* buf, Side& sd) const {
#pragma unroll
    for (int u = 0; u < kSlots; ++u)
      if (off[u] >= 0) buf[off[u]] = v[u];
    if (threadIdx.x < kItems) { sd.id[threadIdx.x] = mine.id; sd.lq[threadIdx.x] = mine.lq; }
  }

  static __device__ __forceinline__ Cand cand(const XentArgs&, int, int q, const Side& sd) { return Cand{sd.id[q], sd.lq[q]}; }
  static __device__ __forceinline__ bool whole(const XentArgs&, int) { return false; }
  static __device__ __forceinline__ bool takes(const XentArgs& a, Cand k, int y) {
    return y >= 0 && k.id != 0 && !(a.remove_hits && k.id == y);       // y = -1: no token
  }
  static __device__ __forceinline__ float logit(Cand k, float acc) { return acc - k.lq; }
  static __device__ __forceinline__ void capture(Cand, int, float, float*, int) {}   // the target is no tile entry
  static __device__ __forceinline__ float prob(Cand k, int, float acc, float l) {     // softmax: the target is no candidate
    const float x = acc - k.lq;
    return __expf(x - l);
  }

  // dE: a workgroup owns slots 64 blockIdx.x + (0..63), walks token split blockIdx.y's tiles and leaves a partial per split
  static __device__ __forceinline__ Cand owner(const XentArgs& a, int slot) {
    const int id = slot_id(a, slot);
    return Cand{id, slot_lq(a, slot, id)};
  }
  static __device__ __forceinline__ int64_t table_row(const XentArgs&, Cand k) { return k.id != 0 ? k.id : -1; }
  static __device__ __forceinline__ void tile_range(const XentArgs& a, int n_tiles, int& tt0, int& tt1) {
    tt0 = (int)((int64_t)blockIdx.y * n_tiles / a.St);
    tt1 = (int)((int64_t)(blockIdx.y + 1) * n_tiles / a.St);
  }
  static __device__ __forceinline__ void store(const XentArgs& a, float* __restrict__ de_part, int slot, int col, float v) {
    if (slot < a.K) de_part[((int64_t)blockIdx.y * a.K + slot) * a.d_item + col] = v;
  }
};

// ---- target logit -----------------------------------------------------------------------------------------------------------
// One thread per position, a fixed-order fma chain over the d_item columns: forward and backward recompute the same bits.
// lse == null (forward): tpos[p] = s_t+.  Otherwise (backward): tpos[p] = g_t+ = d_t (exp(s_t+ - lse_t) - 1), contribution
// row K + p = g_t+ h_t[:d_item] and its key y_t (0 and a zero row at positions without a target).
__global__ void __launch_bounds__(kTargetBlock) sxent_target_kernel(const XentArgs a, const float* __restrict__ lse,
                                                                    const float* __restrict__ d_loss, float* __restrict__ tpos,
                                                                    float* __restrict__ contrib, int64_t* __restrict__ keys) {
  const int64_t p = (int64_t)blockIdx.x * kTargetBlock + threadIdx.x;
  if (p >= a.T) return;
  const int64_t yr = a.targets[p];
  const int y = clamp_id(yr, a.n_items);
  const int di = a.d_item;
  const float* h = a.hidden + p * a.d_out;
  float s = 0.f;
  if (yr != 0) {
    const float* e = a.table + (int64_t)y * di;
    for (int c = 0; c < di; ++c) s = fmaf(h[c], e[c], s);
  }
  if (lse == nullptr) {
    tpos[p] = s;
    return;
  }
  const float g = yr != 0 ? d_loss[p] * (__expf(s - lse[p]) - 1.f) : 0.f;
  tpos[p] = g;
  keys[a.K + p] = yr != 0 ? y : 0;
  float* o = contrib + (a.K + p) * di;
  for (int c = 0; c < di; ++c) o[c] = g * h[c];
}

template <int KS>
__global__ void __launch_bounds__(kThreads) sxent_fwd_kernel(const XentArgs a, float* __restrict__ part_m,
                                                             float* __restrict__ part_s) {
  xent_fwd_body<Negatives, KS>(a, part_m, part_s, nullptr);
}
template <int KS, int NC>
__global__ void __launch_bounds__(kThreads) sxent_dh_kernel(const XentArgs a, const float* __restrict__ lse,
                                                            const float* __restrict__ d_loss, float* __restrict__ dh_part) {
  xent_dh_body<Negatives, KS, NC>(a, lse, d_loss, dh_part);
}
template <int KS, int NC>
__global__ void __launch_bounds__(kThreads) sxent_de_kernel(const XentArgs a, const float* __restrict__ lse,
                                                            const float* __restrict__ d_loss, float* __restrict__ de_part) {
  xent_de_body<Negatives, KS, NC>(a, lse, d_loss, de_part);
}

// the token-split partials of sxent_de_kernel in split order -> one contribution row per slot, and its key
__global__ void __launch_bounds__(256) sxent_de_reduce_kernel(const XentArgs a, int St, const float* __restrict__ de_part,
                                                              float* __restrict__ contrib, int64_t* __restrict__ keys) {
  const int di = a.d_item;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)a.K * di) return;
  const int64_t j = e / di;
  const int col = (int)(e - j * di);
  float s = 0.f;
  for (int sp = 0; sp < St; ++sp) s += de_part[((int64_t)sp * a.K + j) * di + col];
  contrib[j * di + col] = s;
  if (col == 0) keys[j] = slot_id(a, (int)j);
}

}  // namespace
}  // namespace srfrd

using namespace srfrd;

extern "C" int64_t srfrd_sxent_workspace_floats(const srfrd_layout* lay, int B, int L, int K) {
  if (check_layout(lay) != 0 || B <= 0 || L <= 0 || K <= 0) return 0;
  return xent_ws(*lay, B, L, K).total;
}

extern "C" int srfrd_sxent_fwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                               const int64_t* negatives, const float* log_q, int K, int remove_hits, int B, int L,
                               float* token_loss, float* lse, float* stats, float* workspace, int64_t ws_floats, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  XentWs w;
  XentArgs a;
  if (int rc = xent_begin(lay, negatives && token_loss && lse && stats && K > 0, table, hidden, targets, B, L, K, token_loss,
                          lse, nullptr, workspace, ws_floats, st, w, a))
    return rc;
  a.neg = negatives; a.log_q = log_q; a.remove_hits = remove_hits ? 1 : 0;
  hipLaunchKernelGGL(sxent_target_kernel, dim3((unsigned)((a.T + kTargetBlock - 1) / kTargetBlock)), dim3(kTargetBlock), 0, st,
                     a, nullptr, nullptr, workspace + w.tgt, nullptr, nullptr);
  const int tiles = (a.T + kTok - 1) / kTok;
  with_ks((lay->d_item + 3) / 4, [&](auto ks) {
    hipLaunchKernelGGL(sxent_fwd_kernel<decltype(ks)::value>, dim3(tiles, w.S), dim3(kThreads), 0, st, a,
                       workspace + w.part_m, workspace + w.part_s);
  });
  hipLaunchKernelGGL(xent_finalize_kernel, dim3(w.nb_fin), dim3(kFinBlock), 0, st, a.idx, a.count, workspace + w.part_m,
                     workspace + w.part_s, workspace + w.tgt, 1, w.S, (int64_t)a.T, lse, token_loss, workspace + w.bsum);
  hipLaunchKernelGGL(xent_stats_kernel, dim3(1), dim3(256), 0, st, workspace + w.bsum, w.nb_fin, a.count, stats);
  return (int)hipGetLastError();
}

extern "C" int srfrd_sxent_bwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                               const int64_t* negatives, const float* log_q, int K, int remove_hits, const float* lse,
                               const float* d_token_loss, int B, int L, float* d_hidden, float* table_contrib,
                               int64_t* contrib_keys, float* workspace, int64_t ws_floats, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  XentWs w;
  XentArgs a;
  if (int rc = xent_begin(lay, negatives && lse && d_token_loss && d_hidden && table_contrib && contrib_keys && K > 0, table,
                          hidden, targets, B, L, K, nullptr, nullptr, d_hidden, workspace, ws_floats, st, w, a))
    return rc;
  a.neg = negatives; a.log_q = log_q; a.remove_hits = remove_hits ? 1 : 0;
  hipLaunchKernelGGL(sxent_target_kernel, dim3((unsigned)((a.T + kTargetBlock - 1) / kTargetBlock)), dim3(kTargetBlock), 0, st,
                     a, lse, d_token_loss, workspace + w.tgt, table_contrib, contrib_keys);
  const int tiles = (a.T + kTok - 1) / kTok;
  with_ks((lay->d_item + 3) / 4, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    hipLaunchKernelGGL((sxent_dh_kernel<KS, nc_of<KS>()>), dim3(tiles, w.S), dim3(kThreads), 0, st, a, lse, d_token_loss,
                       workspace + w.dh);
    hipLaunchKernelGGL((sxent_de_kernel<KS, nc_of<KS>()>), dim3(a.n_chunks, w.St), dim3(kThreads), 0, st, a, lse,
                       d_token_loss, workspace + w.de);
  });
  hipLaunchKernelGGL(xent_dh_reduce_kernel, dim3((unsigned)(((int64_t)a.T * lay->d_item + 255) / 256)), dim3(256), 0, st, a,
                     workspace + w.dh, (const float*)(workspace + w.tgt), d_hidden);
  hipLaunchKernelGGL(sxent_de_reduce_kernel, dim3((unsigned)(((int64_t)K * lay->d_item + 255) / 256)), dim3(256), 0, st, a,
                     w.St, workspace + w.de, table_contrib, contrib_keys);
  return (int)hipGetLastError();
}
