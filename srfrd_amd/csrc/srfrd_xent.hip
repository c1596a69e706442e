// Full-catalog softmax cross-entropy over the item table, the (tokens x items) logits never written to HBM.
// No reference counterpart: the reference trains with one sampled negative per position (trainer.py:36-38); this is the
// usual SASRec-family alternative.  Semantics: tokens are the positions with targets != 0, candidates the items
// 1..n_items, s_tj = <h_t[:d_item], E[j]>, loss_t = logsumexp_j s_tj - s_t,y.
//
// Every pass works on the compacted token list (the positions with a target, in position order) and on 64-row chunks of
// the item table staged in LDS.  A wave owns 16 tokens (one MFMA row tile); its hidden rows stay in registers as
// v_mfma_f32_16x16x4_f32 fragments for the whole launch.  Logit tiles are formed exactly as the encoder's GEMMs form
// theirs (fp32 matrix cores, a k-ordered product chain), and the same tile arithmetic serves forward and backward.
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

// ---- workspace (floats; every segment 64-aligned) -------------------------------------------------------------------------
struct XentWs {
  int64_t idx, cnt, count, tgt, part_m, part_s, bsum, dh;   // offsets
  int64_t total;
  int S, nb_count, nb_fin;
};
inline int xent_splits(int64_t T, int n_items) {
  const int64_t tiles = (T + kTok - 1) / kTok;
  const int64_t chunks = ((int64_t)n_items + 1 + kItems - 1) / kItems;
  int64_t s = (kSplitTarget + tiles - 1) / tiles;
  s = s < 1 ? 1 : s;
  s = s > chunks ? chunks : s;
  return (int)(s > 64 ? 64 : s);
}
inline XentWs xent_ws(const srfrd_layout& ly, int B, int L) {
  XentWs w;
  const int64_t T = (int64_t)B * L;
  w.S = xent_splits(T, ly.n_items);
  w.nb_count = (int)((T + kCountBlock - 1) / kCountBlock);
  w.nb_fin = (int)((T + kFinBlock - 1) / kFinBlock);
  int64_t o = 0;
  w.idx = o; o += a64(T);
  w.cnt = o; o += a64(w.nb_count);
  w.count = o; o += 64;
  w.tgt = o; o += a64(T);
  const int64_t common = o;
  w.part_m = o; o += a64((int64_t)w.S * T);         // forward only
  w.part_s = o; o += a64((int64_t)w.S * T);
  w.bsum = o; o += a64(w.nb_fin);
  w.dh = common;                                    // backward only: reuses the forward's partials
  const int64_t bwd = common + a64((int64_t)w.S * T * ly.d_item);
  w.total = o > bwd ? o : bwd;
  return w;
}

// ---- shared pieces of the split passes -----------------------------------------------------------------------------------
// A 64-row chunk of the item table is 64 * d_item contiguous floats: thread t copies elements t, t + 256, ... (coalesced).
// The (row, column) of each of its slots is the same for every chunk and is computed once.
struct Stage {
  int off[kSlots];      // LDS offset of slot u, or -1 (beyond the chunk)
  int n;                // elements of a full chunk
};
__device__ __forceinline__ Stage make_stage(int di) {
  Stage s;
  s.n = kItems * di;
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int e = u * kThreads + (int)threadIdx.x;
    const int r = e / di, c = e - r * di;
    s.off[u] = e < s.n ? r * kRS + c : -1;
  }
  return s;
}
__device__ __forceinline__ void stage_fetch(const Stage& s, const float* __restrict__ table, int di, int n_rows_total,
                                            int chunk, float (&v)[kSlots]) {
  const int64_t i0 = (int64_t)chunk * kItems;
  const int64_t rows = (int64_t)n_rows_total - i0;
  const int n = (int)((rows < kItems ? rows : kItems) * di);
  const float* src = table + i0 * di;
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int e = u * kThreads + (int)threadIdx.x;
    v[u] = e < n ? src[e] : 0.f;
  }
}
__device__ __forceinline__ void stage_put(const Stage& s, const float (&v)[kSlots], lds_f* buf) {
#pragma unroll
  for (int u = 0; u < kSlots; ++u)
    if (s.off[u] >= 0) buf[s.off[u]] = v[u];
}

struct SplitArgs {
  const float* table;
  const float* hidden;
  const int64_t* targets;
  const int* idx;
  const int* count;
  int d_item, d_out, n_items, S, n_chunks;
  int T;                // B * L: the row stride of the per-split partials
};

__device__ __forceinline__ void split_range(const SplitArgs& a, int split, int& c0, int& c1) {
  c0 = (int)((int64_t)split * a.n_chunks / a.S);
  c1 = (int)((int64_t)(split + 1) * a.n_chunks / a.S);
}

// ---- forward --------------------------------------------------------------------------------------------------------------
template <int KS>
__global__ void __launch_bounds__(kThreads) xent_fwd_kernel(const SplitArgs a, float* __restrict__ part_m,
                                                            float* __restrict__ part_s, float* __restrict__ tgt) {
  __shared__ float sbuf[2][kItems * kRS];
  const int count = a.count[0];
  const int tok0 = blockIdx.x * kTok;
  if (tok0 >= count) return;
  const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4, w = threadIdx.x >> 6;
  const int tok = tok0 + 16 * w + li;
  const int T = a.T;
  float hf[KS];
  load_hidden<KS>(hf, a.hidden, a.d_out, a.d_item, a.idx, tok, count, lq);
  const int y = tok < count ? clamp_id(a.targets[a.idx[tok]], a.n_items) : -1;
  int c0, c1;
  split_range(a, blockIdx.y, c0, c1);
  lds_f* buf0 = (lds_f*)sbuf[0];
  for (int i = threadIdx.x; i < 2 * kItems * kRS; i += kThreads) buf0[i] = 0.f;
  const Stage st = make_stage(a.d_item);
  float v[kSlots];
  __syncthreads();
  if (c0 < c1) { stage_fetch(st, a.table, a.d_item, a.n_items + 1, c0, v); stage_put(st, v, buf0); }
  __syncthreads();
  float m = -INFINITY, s = 0.f;
  int cur = 0;
  for (int c = c0; c < c1; ++c) {
    if (c + 1 < c1) stage_fetch(st, a.table, a.d_item, a.n_items + 1, c + 1, v);
    f32x4 acc[4];
    logit_tiles_T<KS>(acc, buf0 + cur * kItems * kRS, hf, li, lq);
    const int item0 = c * kItems + 4 * lq;
    const bool full = c > 0 && (c + 1) * kItems <= a.n_items + 1;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int item = item0 + 16 * t + r;
        const float x = acc[t][r];
        if (full || (item >= 1 && item <= a.n_items)) online(m, s, x);
        if (item == y) tgt[tok] = x;          // the one lane of the grid that scores the target
      }
    if (c + 1 < c1) stage_put(st, v, buf0 + (cur ^ 1) * kItems * kRS);
    __syncthreads();
    cur ^= 1;
  }
  // the four lanes of one token (lq = 0..3) hold disjoint item subsets: butterfly merge (both partners compute the same bits)
  {
    float m2 = __shfl_xor(m, 16, 64), s2 = __shfl_xor(s, 16, 64);
    merge(m, s, m2, s2);
    m2 = __shfl_xor(m, 32, 64); s2 = __shfl_xor(s, 32, 64);
    merge(m, s, m2, s2);
  }
  if (lq == 0 && tok < count) {
    part_m[(int64_t)blockIdx.y * T + tok] = m;
    part_s[(int64_t)blockIdx.y * T + tok] = s;
  }
}

__global__ void __launch_bounds__(kFinBlock) xent_finalize_kernel(const int* __restrict__ idx, const int* __restrict__ count_p,
                                                                  const float* __restrict__ part_m, const float* __restrict__ part_s,
                                                                  const float* __restrict__ tgt, int S, int64_t T,
                                                                  float* __restrict__ lse, float* __restrict__ token_loss,
                                                                  float* __restrict__ bsum) {
  __shared__ float sw[kFinBlock / 64];
  const int count = count_p[0];
  const int64_t k = (int64_t)blockIdx.x * kFinBlock + threadIdx.x;
  float loss = 0.f;
  if (k < count) {
    float m = -INFINITY, s = 0.f;
    for (int j = 0; j < S; ++j) merge(m, s, part_m[j * T + k], part_s[j * T + k]);
    const float l = m + __logf(s);
    loss = l - tgt[k];
    const int p = idx[k];
    lse[p] = l;
    token_loss[p] = loss;
  }
  loss = wave_sum(loss);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = loss;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < kFinBlock / 64; ++i) t += sw[i];
    bsum[blockIdx.x] = t;
  }
}

// ---- backward: d_hidden ---------------------------------------------------------------------------------------------------
// P(token li, item 16 t + 4 lq + r) sits where the transposed logit tile left it; as the A operand of P E (A(row, k): lane l
// gives row l & 15, k = l >> 4) register r of tile t is k-step r with k = item 4 lq + r: the tile feeds the product as is.
template <int KS, int NC>
__global__ void __launch_bounds__(kThreads) xent_dh_kernel(const SplitArgs a, const float* __restrict__ lse,
                                                           const float* __restrict__ d_loss, float* __restrict__ dh_part) {
  __shared__ float sbuf[2][kItems * kRS];
  const int count = a.count[0];
  const int tok0 = blockIdx.x * kTok;
  if (tok0 >= count) return;
  const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4, w = threadIdx.x >> 6;
  const int tok = tok0 + 16 * w + li;
  const int T = a.T;
  float hf[KS];
  load_hidden<KS>(hf, a.hidden, a.d_out, a.d_item, a.idx, tok, count, lq);
  int y = -1;
  float l_t = 0.f, g = 0.f;
  if (tok < count) {
    const int p = a.idx[tok];
    y = clamp_id(a.targets[p], a.n_items);
    l_t = lse[p];
    g = d_loss[p];
  }
  int c0, c1;
  split_range(a, blockIdx.y, c0, c1);
  lds_f* buf0 = (lds_f*)sbuf[0];
  for (int i = threadIdx.x; i < 2 * kItems * kRS; i += kThreads) buf0[i] = 0.f;
  const Stage st = make_stage(a.d_item);
  float v[kSlots];
  __syncthreads();
  if (c0 < c1) { stage_fetch(st, a.table, a.d_item, a.n_items + 1, c0, v); stage_put(st, v, buf0); }
  __syncthreads();
  f32x4 dh[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) dh[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  int cur = 0;
  for (int c = c0; c < c1; ++c) {
    if (c + 1 < c1) stage_fetch(st, a.table, a.d_item, a.n_items + 1, c + 1, v);
    const lds_f* b = buf0 + cur * kItems * kRS;
    f32x4 acc[4];
    logit_tiles_T<KS>(acc, b, hf, li, lq);
    const int item0 = c * kItems + 4 * lq;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int item = item0 + 16 * t + r;
        const float p = __expf(acc[t][r] - l_t) - (item == y ? 1.f : 0.f);
        acc[t][r] = (item >= 1 && item <= a.n_items) ? g * p : 0.f;
      }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const lds_f* er = b + (16 * t + 4 * lq + r) * kRS + li;
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) dh[cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[t][r], er[16 * cc], dh[cc], 0, 0, 0);
      }
    if (c + 1 < c1) stage_put(st, v, buf0 + (cur ^ 1) * kItems * kRS);
    __syncthreads();
    cur ^= 1;
  }
  // dh[cc] register r of lane l: token 16 w + 4 lq + r of the tile, column 16 cc + li
#pragma unroll
  for (int cc = 0; cc < NC; ++cc)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int tk = tok0 + 16 * w + 4 * lq + r, col = 16 * cc + li;
      if (tk < count && col < a.d_item) dh_part[((int64_t)blockIdx.y * T + tk) * a.d_item + col] = dh[cc][r];
    }
}

__global__ void __launch_bounds__(256) xent_dh_reduce_kernel(const int* __restrict__ idx, const int* __restrict__ count_p,
                                                             const float* __restrict__ dh_part, int S, int64_t T, int di,
                                                             int d_out, float* __restrict__ d_hidden) {
  const int count = count_p[0];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)count * di) return;
  const int64_t k = e / di;
  const int col = (int)(e - k * di);
  float s = 0.f;
  for (int j = 0; j < S; ++j) s += dh_part[((int64_t)j * T + k) * di + col];
  d_hidden[(int64_t)idx[k] * d_out + col] = s;
}

// ---- backward: dE ---------------------------------------------------------------------------------------------------------
// A workgroup owns 64 items (a wave 16: their rows stay in registers) and walks every token tile in order.  The logit tile
// is formed untransposed, s(token 4 lq + r, item li), so that as the A operand of P^T H it is k-step r with k = token
// 4 lq + r; the B operand H(token, column) comes from the staged token tile.
template <int KS, int NC>
__global__ void __launch_bounds__(kThreads) xent_de_kernel(const SplitArgs a, const float* __restrict__ lse,
                                                           const float* __restrict__ d_loss, float* __restrict__ grad_table,
                                                           int accumulate) {
  __shared__ float sh[kTok * kRS];
  __shared__ float sl[kTok], sg[kTok];
  __shared__ int sy[kTok];
  const int count = a.count[0];
  const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4, w = threadIdx.x >> 6;
  const int di = a.d_item;
  const int item = blockIdx.x * kItems + 16 * w + li;              // this lane's item in the logit tiles
  const bool item_ok = item >= 1 && item <= a.n_items;
  float ef[KS];
  {
    const int64_t row = (int64_t)(item <= a.n_items ? item : a.n_items) * di;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + lq;
      ef[s] = k < di ? a.table[row + k] : 0.f;
    }
  }
  lds_f* H = (lds_f*)sh;
  for (int i = threadIdx.x; i < kTok * kRS; i += kThreads) H[i] = 0.f;
  // staging slots of a token tile: element e = u * 256 + tid is (row e / di, column e % di) of the 64 x d_item tile
  int srow[kSlots], scol[kSlots];
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int e = u * kThreads + (int)threadIdx.x;
    srow[u] = e < kTok * di ? e / di : -1;
    scol[u] = e - (e / di) * di;
  }
  f32x4 de[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) de[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int n_tiles = (count + kTok - 1) / kTok;
  for (int tt = 0; tt < n_tiles; ++tt) {
    const int tok0 = tt * kTok;
    __syncthreads();                              // (the previous tile is consumed)
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      if (srow[u] >= 0) {
        const int tk = tok0 + srow[u];
        H[srow[u] * kRS + scol[u]] = tk < count ? a.hidden[(int64_t)a.idx[tk] * a.d_out + scol[u]] : 0.f;
      }
    }
    if (threadIdx.x < kTok) {
      const int tk = tok0 + threadIdx.x;
      float l = 0.f, g = 0.f;
      int y = -1;
      if (tk < count) {
        const int p = a.idx[tk];
        l = lse[p];
        g = d_loss[p];
        y = clamp_id(a.targets[p], a.n_items);
      }
      sl[threadIdx.x] = l; sg[threadIdx.x] = g; sy[threadIdx.x] = y;
    }
    __syncthreads();
    // logits: acc[j] register r of lane l = s(token 16 j + 4 lq + r, item)
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      float hv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) hv[j] = H[(16 * j + li) * kRS + 4 * s + lq];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[j], ef[s], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 16 * j + 4 * lq + r;
        const float p = __expf(acc[j][r] - sl[q]) - (sy[q] == item ? 1.f : 0.f);
        acc[j][r] = item_ok ? sg[q] * p : 0.f;
      }
    // dE(item 4 lq' + r', column) += sum over tokens: D row = item of A's row (li), k = token, B = H(token, 16 cc + li)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const lds_f* hr = H + (16 * j + 4 * lq + r) * kRS + li;
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) de[cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[j][r], hr[16 * cc], de[cc], 0, 0, 0);
      }
  }
  // de[cc] register r of lane l: item (block, wave) row 4 lq + r, column 16 cc + li
#pragma unroll
  for (int cc = 0; cc < NC; ++cc)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int it = blockIdx.x * kItems + 16 * w + 4 * lq + r, col = 16 * cc + li;
      if (it <= a.n_items && col < di) {
        float* o = grad_table + (int64_t)it * di + col;
        *o = accumulate ? *o + de[cc][r] : de[cc][r];
      }
    }
}

}  // namespace
}  // namespace srfrd

using namespace srfrd;

extern "C" int64_t srfrd_xent_workspace_floats(const srfrd_layout* lay, int B, int L) {
  if (check_layout(lay) != 0 || B <= 0 || L <= 0) return 0;
  return xent_ws(*lay, B, L).total;
}

static int xent_tokens(const XentWs& w, const int64_t* targets, int64_t T, float* ws, float* token_loss, float* lse,
                       hipStream_t st) {
  hipLaunchKernelGGL(xent_count_kernel, dim3(w.nb_count), dim3(kCountBlock), 0, st, targets, T, (int*)(ws + w.cnt));
  hipLaunchKernelGGL(xent_compact_kernel, dim3(w.nb_count), dim3(kCountBlock), 0, st, targets, T, (const int*)(ws + w.cnt),
                     w.nb_count, (int*)(ws + w.idx), ws + w.tgt, (int*)(ws + w.count), token_loss, lse);
  return (int)hipGetLastError();
}

extern "C" int srfrd_xent_fwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets, int B,
                              int L, float* token_loss, float* lse, float* stats, float* workspace, int64_t ws_floats,
                              void* stream) {
  if (int rc = check_layout(lay)) return rc;
  if (!table || !hidden || !targets || !token_loss || !lse || !stats || !workspace || B <= 0 || L <= 0) return SRFRD_E_ARG;
  const XentWs w = xent_ws(*lay, B, L);
  if (ws_floats < w.total) return SRFRD_E_ARG;
  const int64_t T = (int64_t)B * L;
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = xent_tokens(w, targets, T, workspace, token_loss, lse, st)) return rc;
  const int tiles = (int)((T + kTok - 1) / kTok);
  const SplitArgs a{table, hidden, targets, (const int*)(workspace + w.idx), (const int*)(workspace + w.count), lay->d_item,
                    lay->d_out, lay->n_items, w.S, (lay->n_items + 1 + kItems - 1) / kItems, (int)T};
  with_ks((lay->d_item + 3) / 4, [&](auto ks) {
    hipLaunchKernelGGL(xent_fwd_kernel<decltype(ks)::value>, dim3(tiles, w.S), dim3(kThreads), 0, st, a,
                       workspace + w.part_m, workspace + w.part_s, workspace + w.tgt);
  });
  hipLaunchKernelGGL(xent_finalize_kernel, dim3(w.nb_fin), dim3(kFinBlock), 0, st, (const int*)(workspace + w.idx),
                     (const int*)(workspace + w.count), workspace + w.part_m, workspace + w.part_s, workspace + w.tgt, w.S, T, lse, token_loss, workspace + w.bsum);
  hipLaunchKernelGGL(xent_stats_kernel, dim3(1), dim3(256), 0, st, workspace + w.bsum, w.nb_fin,
                     (const int*)(workspace + w.count), stats);
  return (int)hipGetLastError();
}

extern "C" int srfrd_xent_bwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                              const float* lse, const float* d_token_loss, int B, int L, float* d_hidden, float* grad_table,
                              int accumulate, float* workspace, int64_t ws_floats, void* stream) {
  if (int rc = check_layout(lay)) return rc;
  if (!table || !hidden || !targets || !lse || !d_token_loss || !d_hidden || !grad_table || !workspace || B <= 0 || L <= 0)
    return SRFRD_E_ARG;
  const XentWs w = xent_ws(*lay, B, L);
  if (ws_floats < w.total) return SRFRD_E_ARG;
  const int64_t T = (int64_t)B * L;
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = xent_tokens(w, targets, T, workspace, nullptr, nullptr, st)) return rc;
  if (int rc = zero_floats(d_hidden, T * lay->d_out, st)) return rc;
  const int tiles = (int)((T + kTok - 1) / kTok);
  const int n_chunks = (lay->n_items + 1 + kItems - 1) / kItems;
  const SplitArgs a{table, hidden, targets, (const int*)(workspace + w.idx), (const int*)(workspace + w.count), lay->d_item,
                    lay->d_out, lay->n_items, w.S, n_chunks, (int)T};
  with_ks((lay->d_item + 3) / 4, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    hipLaunchKernelGGL((xent_dh_kernel<KS, nc_of<KS>()>), dim3(tiles, w.S), dim3(kThreads), 0, st, a, lse, d_token_loss,
                       workspace + w.dh);
    hipLaunchKernelGGL((xent_de_kernel<KS, nc_of<KS>()>), dim3(n_chunks), dim3(kThreads), 0, st, a, lse, d_token_loss,
                       grad_table, accumulate);
  });
  hipLaunchKernelGGL(xent_dh_reduce_kernel, dim3((unsigned)((T * lay->d_item + 255) / 256)), dim3(256), 0, st,
                     (const int*)(workspace + w.idx), (const int*)(workspace + w.count), workspace + w.dh, w.S, T, lay->d_item, lay->d_out, d_hidden);
  return (int)hipGetLastError();
}
