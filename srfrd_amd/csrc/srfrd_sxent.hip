// Sampled softmax cross-entropy with shared negatives: every token is scored against its own target and one set of K
// sampled items shared by the whole batch, the (tokens x (1 + K)) logits never written to HBM.  No reference counterpart
// (the reference trains with one sampled negative per position, trainer.py:36-38).  Semantics: tokens are the positions
// with targets != 0; s_t+ = <h_t[:d_item], E[y_t]>; negative slot j has s_tj = <h_t[:d_item], E[n_j]> - log_q[j] (nothing
// subtracted without log_q); loss_t = logsumexp({s_t+} u {s_tj : n_j != 0, n_j != y_t if remove_hits}) - s_t+.
//
// The machinery is that of srfrd_xent.hip (srfrd_xent_common.h): the compacted token list, 16-token register tiles on
// v_mfma_f32_16x16x4_f32, an online (max, sum of exp) per token, fixed-order merges of split partials.  Where xent streams
// contiguous 64-row chunks of the table, these kernels stream 64-slot chunks of the negatives, gathering the rows E[n_j]
// by id into LDS with the slot ids and log_q beside them; id-0 slots and accidental hits are masked by a compare against
// the token's target.  The target logit is one fixed-order dot product per token (sxent_target_kernel), not a tile entry.
//
//   forward   xent_count / xent_compact   token list
//             sxent_target_kernel         s_t+ per position
//             sxent_fwd_kernel            (token tile, slot split): online (max, sum of exp) per token
//             sxent_finalize_kernel       (s_t+, 1) merged with the splits in split order -> lse, token loss, block sums
//             xent_stats_kernel           the block sums in block order -> stats {sum, count}
//   backward  xent_count / xent_compact   token list
//             sxent_target_kernel         g_t+ = d_t (softmax_t+ - 1), its table contribution row g_t+ h_t and key y_t
//             sxent_dh_kernel             (token tile, slot split): P = d_t softmax in-tile, dH partial = P E_neg
//             sxent_dh_reduce_kernel      the split partials in split order, then g_t+ E[y_t] -> d_hidden
//             sxent_de_kernel             (64-slot chunk, token split): dE partial = P^T H over its token tiles in order
//             sxent_de_reduce_kernel      the token-split partials in split order -> one contribution row per slot, its key
// The table gradient is left as (K + B L) contribution rows with their item ids as keys, which the caller sums per item
// with srfrd_table_reduce after a stable sort.  No float atomics anywhere: two identical calls are bitwise identical.

#include "srfrd_xent_common.h"

namespace srfrd {
namespace {

constexpr int kTargetBlock = 256;

// ---- workspace (floats; every segment 64-aligned) -------------------------------------------------------------------------
struct SxentWs {
  int64_t idx, cnt, count, tpos, part_m, part_s, bsum, dh, de;   // offsets
  int64_t total;
  int S, St, nb_count, nb_fin;
};
// split count of a pass over `parts` units whose other dimension has `tiles` workgroups: aim at kSplitTarget workgroups
inline int sxent_splits(int64_t tiles, int64_t parts) {
  int64_t s = (kSplitTarget + tiles - 1) / tiles;
  s = s < 1 ? 1 : s;
  s = s > parts ? parts : s;
  return (int)(s > 64 ? 64 : s);
}
inline SxentWs sxent_ws(const srfrd_layout& ly, int B, int L, int K) {
  SxentWs w;
  const int64_t T = (int64_t)B * L;
  const int64_t tiles = (T + kTok - 1) / kTok, chunks = ((int64_t)K + kItems - 1) / kItems;
  w.S = sxent_splits(tiles, chunks);           // slot splits of the forward and of the dH pass
  w.St = sxent_splits(chunks, tiles);          // token splits of the dE pass
  w.nb_count = (int)((T + kCountBlock - 1) / kCountBlock);
  w.nb_fin = (int)((T + kFinBlock - 1) / kFinBlock);
  int64_t o = 0;
  w.idx = o; o += a64(T);
  w.cnt = o; o += a64(w.nb_count);
  w.count = o; o += 64;
  w.tpos = o; o += a64(T);                          // forward: s_t+; backward: g_t+ (by position)
  const int64_t common = o;
  w.part_m = o; o += a64((int64_t)w.S * T);         // forward only
  w.part_s = o; o += a64((int64_t)w.S * T);
  w.bsum = o; o += a64(w.nb_fin);
  int64_t b = common;                               // backward only: reuses the forward's partials
  w.dh = b; b += a64((int64_t)w.S * T * ly.d_item);
  w.de = b; b += a64((int64_t)w.St * K * ly.d_item);
  w.total = o > b ? o : b;
  return w;
}

struct SArgs {
  const float* table;
  const float* hidden;
  const int64_t* targets;
  const int64_t* neg;
  const float* log_q;   // may be null
  const int* idx;
  const int* count;
  int d_item, d_out, n_items, K, S, n_chunks;
  int T;                // B * L: the row stride of the per-split partials
  int remove_hits;
};

__device__ __forceinline__ void chunk_range(const SArgs& a, int split, int& c0, int& c1) {
  c0 = (int)((int64_t)split * a.n_chunks / a.S);
  c1 = (int)((int64_t)(split + 1) * a.n_chunks / a.S);
}

// slot j's item id (clamped; 0 for an unused slot or j >= K) and its log-Q correction (0 where it takes no part)
__device__ __forceinline__ int slot_id(const SArgs& a, int j) { return j < a.K ? clamp_id(a.neg[j], a.n_items) : 0; }
__device__ __forceinline__ float slot_lq(const SArgs& a, int j, int id) {
  return (a.log_q != nullptr && id != 0) ? a.log_q[j] : 0.f;
}
// whether slot id `id` is a candidate of a token with (clamped) target y
__device__ __forceinline__ bool takes_part(int id, int y, int remove_hits) { return id != 0 && !(remove_hits && id == y); }

// ---- gathered staging of a 64-slot chunk ----------------------------------------------------------------------------------
// Element e = u * 256 + tid of the chunk is (slot row e / d_item, column e % d_item), read from E[n_j] (zeros for unused
// slots and past K).  Threads 0..63 also fetch their slot's id and log_q.
struct Gather {
  int off[kSlots];      // LDS offset of element u, or -1 (beyond the chunk)
  int row[kSlots];      // its slot row in the chunk
  int col[kSlots];
};
__device__ __forceinline__ Gather make_gather(int di) {
  Gather g;
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int e = u * kThreads + (int)threadIdx.x;
    const int r = e / di, c = e - r * di;
    g.off[u] = e < kItems * di ? r * kRS + c : -1;
    g.row[u] = r;
    g.col[u] = c;
  }
  return g;
}
struct Staged {
  float v[kSlots];
  int id;
  float lq;
};
__device__ __forceinline__ void gather_fetch(const Gather& g, const SArgs& a, int chunk, Staged& s) {
  const int j0 = chunk * kItems;
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    float x = 0.f;
    if (g.off[u] >= 0) {
      const int id = slot_id(a, j0 + g.row[u]);
      if (id != 0) x = a.table[(int64_t)id * a.d_item + g.col[u]];
    }
    s.v[u] = x;
  }
  if (threadIdx.x < kItems) {
    const int j = j0 + (int)threadIdx.x;
    s.id = slot_id(a, j);
    s.lq = slot_lq(a, j, s.id);
  }
}
__device__ __forceinline__ void gather_put(const Gather& g, const Staged& s, lds_f* buf, int* sid, float* slq) {
#pragma unroll
  for (int u = 0; u < kSlots; ++u)
    if (g.off[u] >= 0) buf[g.off[u]] = s.v[u];
  if (threadIdx.x < kItems) { sid[threadIdx.x] = s.id; slq[threadIdx.x] = s.lq; }
}

// ---- target logit -----------------------------------------------------------------------------------------------------------
// One thread per position, a fixed-order fma chain over the d_item columns: forward and backward recompute the same bits.
// lse == null (forward): tpos[p] = s_t+.  Otherwise (backward): tpos[p] = g_t+ = d_t (exp(s_t+ - lse_t) - 1), contribution
// row K + p = g_t+ h_t[:d_item] and its key y_t (0 and a zero row at positions without a target).
__global__ void __launch_bounds__(kTargetBlock) sxent_target_kernel(const SArgs a, const float* __restrict__ lse,
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

// ---- forward --------------------------------------------------------------------------------------------------------------
template <int KS>
__global__ void __launch_bounds__(kThreads) sxent_fwd_kernel(const SArgs a, float* __restrict__ part_m,
                                                             float* __restrict__ part_s) {
  __shared__ float sbuf[2][kItems * kRS];
  __shared__ int sid[2][kItems];
  __shared__ float slq[2][kItems];
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
  chunk_range(a, blockIdx.y, c0, c1);
  lds_f* buf0 = (lds_f*)sbuf[0];
  for (int i = threadIdx.x; i < 2 * kItems * kRS; i += kThreads) buf0[i] = 0.f;
  const Gather gt = make_gather(a.d_item);
  Staged nx;
  __syncthreads();
  if (c0 < c1) { gather_fetch(gt, a, c0, nx); gather_put(gt, nx, buf0, sid[0], slq[0]); }
  __syncthreads();
  float m = -INFINITY, s = 0.f;
  int cur = 0;
  for (int c = c0; c < c1; ++c) {
    if (c + 1 < c1) gather_fetch(gt, a, c + 1, nx);
    f32x4 acc[4];
    logit_tiles_T<KS>(acc, buf0 + cur * kItems * kRS, hf, li, lq);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 16 * t + 4 * lq + r;
        const float x = acc[t][r] - slq[cur][q];
        if (takes_part(sid[cur][q], y, a.remove_hits)) online(m, s, x);
      }
    if (c + 1 < c1) gather_put(gt, nx, buf0 + (cur ^ 1) * kItems * kRS, sid[cur ^ 1], slq[cur ^ 1]);
    __syncthreads();
    cur ^= 1;
  }
  // the four lanes of one token (lq = 0..3) hold disjoint slot subsets: butterfly merge (both partners compute the same bits)
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

__global__ void __launch_bounds__(kFinBlock) sxent_finalize_kernel(const int* __restrict__ idx, const int* __restrict__ count_p,
                                                                   const float* __restrict__ part_m, const float* __restrict__ part_s,
                                                                   const float* __restrict__ tpos, int S, int64_t T,
                                                                   float* __restrict__ lse, float* __restrict__ token_loss,
                                                                   float* __restrict__ bsum) {
  __shared__ float sw[kFinBlock / 64];
  const int count = count_p[0];
  const int64_t k = (int64_t)blockIdx.x * kFinBlock + threadIdx.x;
  float loss = 0.f;
  if (k < count) {
    const int p = idx[k];
    const float tg = tpos[p];
    float m = tg, s = 1.f;                          // the target's own term first, then the splits in split order
    for (int j = 0; j < S; ++j) merge(m, s, part_m[j * T + k], part_s[j * T + k]);
    const float l = m + __logf(s);
    loss = l - tg;
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
// As xent_dh_kernel: the transposed logit tile, turned into P = d_t softmax_tj in place, is the A operand of P E_neg.
template <int KS, int NC>
__global__ void __launch_bounds__(kThreads) sxent_dh_kernel(const SArgs a, const float* __restrict__ lse,
                                                            const float* __restrict__ d_loss, float* __restrict__ dh_part) {
  __shared__ float sbuf[2][kItems * kRS];
  __shared__ int sid[2][kItems];
  __shared__ float slq[2][kItems];
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
  const bool tok_ok = tok < count;
  int c0, c1;
  chunk_range(a, blockIdx.y, c0, c1);
  lds_f* buf0 = (lds_f*)sbuf[0];
  for (int i = threadIdx.x; i < 2 * kItems * kRS; i += kThreads) buf0[i] = 0.f;
  const Gather gt = make_gather(a.d_item);
  Staged nx;
  __syncthreads();
  if (c0 < c1) { gather_fetch(gt, a, c0, nx); gather_put(gt, nx, buf0, sid[0], slq[0]); }
  __syncthreads();
  f32x4 dh[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) dh[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  int cur = 0;
  for (int c = c0; c < c1; ++c) {
    if (c + 1 < c1) gather_fetch(gt, a, c + 1, nx);
    const lds_f* b = buf0 + cur * kItems * kRS;
    f32x4 acc[4];
    logit_tiles_T<KS>(acc, b, hf, li, lq);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 16 * t + 4 * lq + r;
        const float x = acc[t][r] - slq[cur][q];
        acc[t][r] = (tok_ok && takes_part(sid[cur][q], y, a.remove_hits)) ? g * __expf(x - l_t) : 0.f;
      }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const lds_f* er = b + (16 * t + 4 * lq + r) * kRS + li;
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) dh[cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[t][r], er[16 * cc], dh[cc], 0, 0, 0);
      }
    if (c + 1 < c1) gather_put(gt, nx, buf0 + (cur ^ 1) * kItems * kRS, sid[cur ^ 1], slq[cur ^ 1]);
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

__global__ void __launch_bounds__(256) sxent_dh_reduce_kernel(const SArgs a, const float* __restrict__ dh_part,
                                                              const float* __restrict__ gpos, float* __restrict__ d_hidden) {
  const int count = a.count[0];
  const int di = a.d_item;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)count * di) return;
  const int64_t k = e / di;
  const int col = (int)(e - k * di);
  const int64_t T = a.T;
  float s = 0.f;
  for (int j = 0; j < a.S; ++j) s += dh_part[((int64_t)j * T + k) * di + col];
  const int p = a.idx[k];
  const int y = clamp_id(a.targets[p], a.n_items);
  s = fmaf(gpos[p], a.table[(int64_t)y * di + col], s);
  d_hidden[(int64_t)p * a.d_out + col] = s;
}

// ---- backward: the negatives' dE ------------------------------------------------------------------------------------------
// A workgroup owns 64 slots (a wave 16: their rows E[n_j] stay in registers) and walks its token split's tiles in order.  As
// xent_de_kernel: the logit tile is formed untransposed, s(token 4 lq + r, slot li), the A operand of P^T H as it stands.
template <int KS, int NC>
__global__ void __launch_bounds__(kThreads) sxent_de_kernel(const SArgs a, int St, const float* __restrict__ lse,
                                                            const float* __restrict__ d_loss, float* __restrict__ de_part) {
  __shared__ float sh[kTok * kRS];
  __shared__ float sl[kTok], sg[kTok];
  __shared__ int sy[kTok];
  const int count = a.count[0];
  const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4, w = threadIdx.x >> 6;
  const int di = a.d_item;
  const int slot = blockIdx.x * kItems + 16 * w + li;              // this lane's slot in the logit tiles
  const int id = slot_id(a, slot);
  const float lqj = slot_lq(a, slot, id);
  float ef[KS];
  {
    const int64_t row = (int64_t)id * di;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + lq;
      ef[s] = (id != 0 && k < di) ? a.table[row + k] : 0.f;
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
  const int tt0 = (int)((int64_t)blockIdx.y * n_tiles / St), tt1 = (int)((int64_t)(blockIdx.y + 1) * n_tiles / St);
  for (int tt = tt0; tt < tt1; ++tt) {
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
      int y = -1;                                 // -1: no token here
      if (tk < count) {
        const int p = a.idx[tk];
        l = lse[p];
        g = d_loss[p];
        y = clamp_id(a.targets[p], a.n_items);
      }
      sl[threadIdx.x] = l; sg[threadIdx.x] = g; sy[threadIdx.x] = y;
    }
    __syncthreads();
    // logits: acc[j] register r of lane l = s(token 16 j + 4 lq + r, slot)
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
        const float x = acc[j][r] - lqj;
        acc[j][r] = (sy[q] >= 0 && takes_part(id, sy[q], a.remove_hits)) ? sg[q] * __expf(x - sl[q]) : 0.f;
      }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const lds_f* hr = H + (16 * j + 4 * lq + r) * kRS + li;
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) de[cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[j][r], hr[16 * cc], de[cc], 0, 0, 0);
      }
  }
  // de[cc] register r of lane l: slot (block, wave) row 4 lq + r, column 16 cc + li; written even for an empty token range
#pragma unroll
  for (int cc = 0; cc < NC; ++cc)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int sj = blockIdx.x * kItems + 16 * w + 4 * lq + r, col = 16 * cc + li;
      if (sj < a.K && col < di) de_part[((int64_t)blockIdx.y * a.K + sj) * di + col] = de[cc][r];
    }
}

__global__ void __launch_bounds__(256) sxent_de_reduce_kernel(const SArgs a, int St, const float* __restrict__ de_part,
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
  return sxent_ws(*lay, B, L, K).total;
}

static int sxent_tokens(const SxentWs& w, const int64_t* targets, int64_t T, float* ws, float* token_loss, float* lse,
                        hipStream_t st) {
  hipLaunchKernelGGL(xent_count_kernel, dim3(w.nb_count), dim3(kCountBlock), 0, st, targets, T, (int*)(ws + w.cnt));
  hipLaunchKernelGGL(xent_compact_kernel, dim3(w.nb_count), dim3(kCountBlock), 0, st, targets, T, (const int*)(ws + w.cnt),
                     w.nb_count, (int*)(ws + w.idx), ws + w.tpos, (int*)(ws + w.count), token_loss, lse);
  return (int)hipGetLastError();
}

static SArgs sxent_args(const srfrd_layout* lay, const SxentWs& w, const float* table, const float* hidden,
                        const int64_t* targets, const int64_t* negatives, const float* log_q, int K, int remove_hits,
                        int64_t T, const float* ws) {
  return SArgs{table, hidden, targets, negatives, log_q, (const int*)(ws + w.idx), (const int*)(ws + w.count), lay->d_item,
               lay->d_out, lay->n_items, K, w.S, (K + kItems - 1) / kItems, (int)T, remove_hits ? 1 : 0};
}

extern "C" int srfrd_sxent_fwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                               const int64_t* negatives, const float* log_q, int K, int remove_hits, int B, int L,
                               float* token_loss, float* lse, float* stats, float* workspace, int64_t ws_floats, void* stream) {
  if (int rc = check_layout(lay)) return rc;
  if (!table || !hidden || !targets || !negatives || !token_loss || !lse || !stats || !workspace || K <= 0 || B <= 0 || L <= 0)
    return SRFRD_E_ARG;
  const SxentWs w = sxent_ws(*lay, B, L, K);
  if (ws_floats < w.total) return SRFRD_E_ARG;
  const int64_t T = (int64_t)B * L;
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = sxent_tokens(w, targets, T, workspace, token_loss, lse, st)) return rc;
  const SArgs a = sxent_args(lay, w, table, hidden, targets, negatives, log_q, K, remove_hits, T, workspace);
  hipLaunchKernelGGL(sxent_target_kernel, dim3((unsigned)((T + kTargetBlock - 1) / kTargetBlock)), dim3(kTargetBlock), 0, st, a,
                     nullptr, nullptr, workspace + w.tpos, nullptr, nullptr);
  const int tiles = (int)((T + kTok - 1) / kTok);
  with_ks((lay->d_item + 3) / 4, [&](auto ks) {
    hipLaunchKernelGGL(sxent_fwd_kernel<decltype(ks)::value>, dim3(tiles, w.S), dim3(kThreads), 0, st, a,
                       workspace + w.part_m, workspace + w.part_s);
  });
  hipLaunchKernelGGL(sxent_finalize_kernel, dim3(w.nb_fin), dim3(kFinBlock), 0, st, (const int*)(workspace + w.idx),
                     (const int*)(workspace + w.count), workspace + w.part_m, workspace + w.part_s, workspace + w.tpos, w.S, T,
                     lse, token_loss, workspace + w.bsum);
  hipLaunchKernelGGL(xent_stats_kernel, dim3(1), dim3(256), 0, st, workspace + w.bsum, w.nb_fin,
                     (const int*)(workspace + w.count), stats);
  return (int)hipGetLastError();
}

extern "C" int srfrd_sxent_bwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                               const int64_t* negatives, const float* log_q, int K, int remove_hits, const float* lse,
                               const float* d_token_loss, int B, int L, float* d_hidden, float* table_contrib,
                               int64_t* contrib_keys, float* workspace, int64_t ws_floats, void* stream) {
  if (int rc = check_layout(lay)) return rc;
  if (!table || !hidden || !targets || !negatives || !lse || !d_token_loss || !d_hidden || !table_contrib || !contrib_keys ||
      !workspace || K <= 0 || B <= 0 || L <= 0)
    return SRFRD_E_ARG;
  const SxentWs w = sxent_ws(*lay, B, L, K);
  if (ws_floats < w.total) return SRFRD_E_ARG;
  const int64_t T = (int64_t)B * L;
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = sxent_tokens(w, targets, T, workspace, nullptr, nullptr, st)) return rc;
  if (int rc = zero_floats(d_hidden, T * lay->d_out, st)) return rc;
  const SArgs a = sxent_args(lay, w, table, hidden, targets, negatives, log_q, K, remove_hits, T, workspace);
  hipLaunchKernelGGL(sxent_target_kernel, dim3((unsigned)((T + kTargetBlock - 1) / kTargetBlock)), dim3(kTargetBlock), 0, st, a,
                     lse, d_token_loss, workspace + w.tpos, table_contrib, contrib_keys);
  const int tiles = (int)((T + kTok - 1) / kTok);
  with_ks((lay->d_item + 3) / 4, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    hipLaunchKernelGGL((sxent_dh_kernel<KS, nc_of<KS>()>), dim3(tiles, w.S), dim3(kThreads), 0, st, a, lse, d_token_loss,
                       workspace + w.dh);
    hipLaunchKernelGGL((sxent_de_kernel<KS, nc_of<KS>()>), dim3(a.n_chunks, w.St), dim3(kThreads), 0, st, a, w.St, lse,
                       d_token_loss, workspace + w.de);
  });
  hipLaunchKernelGGL(sxent_dh_reduce_kernel, dim3((unsigned)((T * lay->d_item + 255) / 256)), dim3(256), 0, st, a,
                     workspace + w.dh, workspace + w.tpos, d_hidden);
  hipLaunchKernelGGL(sxent_de_reduce_kernel, dim3((unsigned)(((int64_t)K * lay->d_item + 255) / 256)), dim3(256), 0, st, a,
                     w.St, workspace + w.de, table_contrib, contrib_keys);
  return (int)hipGetLastError();
}
