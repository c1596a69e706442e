// The softmax cross-entropy loss head, written once for both candidate sources: srfrd_xent.hip (the whole catalog) and
// srfrd_sxent.hip (K negatives shared by the batch).  Both work on the compacted token list (the positions with a target, in
// position order) with 16-token register tiles on v_mfma_f32_16x16x4_f32, an online (max, sum of exp) per token, and
// fixed-order merges of their split partials.  A wave owns 16 tokens (one MFMA row tile); its hidden rows stay in registers
// as MFMA fragments for the whole launch, and the candidates stream past them in 64-row chunks staged in LDS.
//
// The three streaming passes (xent_fwd_body, xent_dh_body, xent_de_body) are function templates over a policy type Src that
// the two .hip files define and their __global__ kernels instantiate.  Src supplies only what differs between the sources:
//   Src(a), fetch(a, c), put(buf, side)   chunk c from HBM into registers, then into LDS (Src::Side: its per-slot LDS arrays)
//   Cand, cand(a, c, q, side), owner(a, row)   what entry q of chunk c / row `row` of the dE grid is scored as
//   whole(a, c)                           every entry of chunk c takes part for every token (no per-entry test)
//   takes(a, k, y), logit(k, acc), capture(k, y, x, tgt, tok), prob(k, y, acc, l)   the per-entry rule
//   table_row(a, k), tile_range(a, n, t0, t1), store(a, out, row, col, v)   the dE pass: the owner's table row (-1: none),
//                                                                  its token tiles, and where its gradient row goes
// takes and prob stay apart, and the passes read a token's d_loss inside the mask: a single rule that took the token's values
// as arguments had them loaded for every entry, masked or not (the catalog's dE pass: 20 more VGPRs, a wave less at d_item <= 4).
// The small kernels around them (token list, finalize, dH reduce, stats) and the launchers' preamble are shared as they are.
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

// ---- workspace (floats; every segment 64-aligned) -------------------------------------------------------------------------
struct XentWs {
  int64_t idx, cnt, count, tgt, part_m, part_s, bsum, dh, de;   // offsets
  int64_t total;
  int S, St, n_chunks, nb_count, nb_fin;
};
// split count of a pass over `parts` units whose other dimension has `tiles` workgroups: aim at kSplitTarget workgroups
inline int xent_splits(int64_t tiles, int64_t parts) {
  int64_t s = (kSplitTarget + tiles - 1) / tiles;
  s = s < 1 ? 1 : s;
  s = s > parts ? parts : s;
  return (int)(s > 64 ? 64 : s);
}
// K shared negatives, or K = 0: the whole catalog (rows 0..n_items; no token splits and no partials of the dE pass)
inline XentWs xent_ws(const srfrd_layout& ly, int B, int L, int K) {
  XentWs w;
  const int64_t T = (int64_t)B * L;
  const int64_t tiles = (T + kTok - 1) / kTok;
  w.n_chunks = (int)(((K > 0 ? (int64_t)K : (int64_t)ly.n_items + 1) + kItems - 1) / kItems);
  w.S = xent_splits(tiles, w.n_chunks);                   // candidate splits of the forward and of the dH pass
  w.St = K > 0 ? xent_splits(w.n_chunks, tiles) : 1;      // token splits of the dE pass
  w.nb_count = (int)((T + kCountBlock - 1) / kCountBlock);
  w.nb_fin = (int)((T + kFinBlock - 1) / kFinBlock);
  int64_t o = 0;
  w.idx = o; o += a64(T);
  w.cnt = o; o += a64(w.nb_count);
  w.count = o; o += 64;
  w.tgt = o; o += a64(T);                           // the target logit s_t+ (catalog: by token; sampled: by position, and
  const int64_t common = o;                         // g_t+ in the backward)
  w.part_m = o; o += a64((int64_t)w.S * T);         // forward only
  w.part_s = o; o += a64((int64_t)w.S * T);
  w.bsum = o; o += a64(w.nb_fin);
  int64_t b = common;                               // backward only: reuses the forward's partials
  w.dh = b; b += a64((int64_t)w.S * T * ly.d_item);
  w.de = b; b += a64((int64_t)w.St * K * ly.d_item);
  w.total = o > b ? o : b;
  return w;
}

struct XentArgs {
  const float* table;
  const float* hidden;
  const int64_t* targets;
  const int* idx;
  const int* count;
  int d_item, d_out, n_items, S, n_chunks;
  int T;                // B * L: the row stride of the per-split partials
  // the catalog's dE pass
  int accumulate;
  // shared negatives only
  const int64_t* neg;
  const float* log_q;   // may be null
  int K, St, remove_hits;
};

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

// ---- the (token tile, candidate split) passes: forward and dH --------------------------------------------------------------
struct TokLane {        // a lane of a token-tile workgroup: wave w holds tokens tok0 + 16 w + (0..15), this lane token `tok`
  int count, tok0, li, lq, w, tok;
  __device__ __forceinline__ explicit TokLane(const XentArgs& a) {
    count = a.count[0];
    tok0 = blockIdx.x * kTok;
    const int lane = threadIdx.x & 63;
    li = lane & 15; lq = lane >> 4; w = threadIdx.x >> 6;
    tok = tok0 + 16 * w + li;
  }
};

// The chunks of split blockIdx.y, double-buffered through LDS: while chunk c + 1 is in flight to registers, use(acc, buf, c,
// side) gets chunk c's transposed logit tiles (register r of tile t: entry q = 16 t + 4 lq + r of the chunk), its staged rows
// and its side arrays.
template <class Src, int KS, class F>
__device__ __forceinline__ void stream_chunks(const XentArgs& a, const TokLane& tl, F&& use) {
  __shared__ float sbuf[2][kItems * kRS];
  __shared__ typename Src::Side side[2];
  float hf[KS];
  load_hidden<KS>(hf, a.hidden, a.d_out, a.d_item, a.idx, tl.tok, tl.count, tl.lq);
  const int c0 = (int)((int64_t)blockIdx.y * a.n_chunks / a.S), c1 = (int)((int64_t)(blockIdx.y + 1) * a.n_chunks / a.S);
  lds_f* buf0 = (lds_f*)sbuf[0];
  for (int i = threadIdx.x; i < 2 * kItems * kRS; i += kThreads) buf0[i] = 0.f;
  Src src(a);
  __syncthreads();
  if (c0 < c1) { src.fetch(a, c0); src.put(buf0, side[0]); }
  __syncthreads();
  int cur = 0;
  for (int c = c0; c < c1; ++c) {
    if (c + 1 < c1) src.fetch(a, c + 1);
    const lds_f* b = buf0 + cur * kItems * kRS;
    f32x4 acc[4];
    logit_tiles_T<KS>(acc, b, hf, tl.li, tl.lq);
    use(acc, b, c, side[cur]);
    if (c + 1 < c1) src.put(buf0 + (cur ^ 1) * kItems * kRS, side[cur ^ 1]);
    __syncthreads();
    cur ^= 1;
  }
}

// forward: online (max, sum of exp) per token over the split's candidates -> part_m, part_s [split][token]
template <class Src, int KS>
__device__ __forceinline__ void xent_fwd_body(const XentArgs& a, float* __restrict__ part_m, float* __restrict__ part_s,
                                              float* __restrict__ tgt) {
  const TokLane tl(a);
  if (tl.tok0 >= tl.count) return;
  const int y = tl.tok < tl.count ? clamp_id(a.targets[a.idx[tl.tok]], a.n_items) : -1;
  float m = -INFINITY, s = 0.f;
  stream_chunks<Src, KS>(a, tl, [&](f32x4 (&acc)[4], const lds_f*, int c, const typename Src::Side& sd) {
    const bool whole = Src::whole(a, c);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const auto k = Src::cand(a, c, 16 * t + 4 * tl.lq + r, sd);
        const float x = Src::logit(k, acc[t][r]);
        if (whole || Src::takes(a, k, y)) online(m, s, x);
        Src::capture(k, y, x, tgt, tl.tok);
      }
  });
  // the four lanes of one token (lq = 0..3) hold disjoint candidate subsets: butterfly merge (both partners compute the same
  // bits)
  {
    float m2 = __shfl_xor(m, 16, 64), s2 = __shfl_xor(s, 16, 64);
    merge(m, s, m2, s2);
    m2 = __shfl_xor(m, 32, 64); s2 = __shfl_xor(s, 32, 64);
    merge(m, s, m2, s2);
  }
  if (tl.lq == 0 && tl.tok < tl.count) {
    part_m[(int64_t)blockIdx.y * a.T + tl.tok] = m;
    part_s[(int64_t)blockIdx.y * a.T + tl.tok] = s;
  }
}

// target_apart = 0 (catalog): the forward captured the target logit among the candidates, tgt[token].  1 (sampled): it is
// tgt[position] and a term of its own, merged first; then the splits in split order either way.
__global__ void __launch_bounds__(kFinBlock) xent_finalize_kernel(const int* __restrict__ idx, const int* __restrict__ count_p,
                                                                  const float* __restrict__ part_m, const float* __restrict__ part_s,
                                                                  const float* __restrict__ tgt, int target_apart, int S,
                                                                  int64_t T, float* __restrict__ lse,
                                                                  float* __restrict__ token_loss, float* __restrict__ bsum) {
  __shared__ float sw[kFinBlock / 64];
  const int count = count_p[0];
  const int64_t k = (int64_t)blockIdx.x * kFinBlock + threadIdx.x;
  float loss = 0.f;
  if (k < count) {
    const int p = idx[k];
    const float tg = tgt[target_apart ? p : k];
    float m = -INFINITY, s = 0.f;
    if (target_apart) { m = tg; s = 1.f; }
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

// dH: the transposed logit tile becomes P = g Src::prob(...) in place.  P(token li, entry 16 t + 4 lq + r) sits where the
// logits were; as the A operand of P E (A(row, k): lane l gives row l & 15, k = l >> 4) register r of tile t is k-step r with
// k = entry 4 lq + r: the tile feeds the product as is.  dH partial = P E -> dh_part [split][token][d_item]
template <class Src, int KS, int NC>
__device__ __forceinline__ void xent_dh_body(const XentArgs& a, const float* __restrict__ lse,
                                             const float* __restrict__ d_loss, float* __restrict__ dh_part) {
  const TokLane tl(a);
  if (tl.tok0 >= tl.count) return;
  int y = -1;                                     // -1: no token in this lane
  float l_t = 0.f, g = 0.f;
  if (tl.tok < tl.count) {
    const int p = a.idx[tl.tok];
    y = clamp_id(a.targets[p], a.n_items);
    l_t = lse[p];
    g = d_loss[p];
  }
  f32x4 dh[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) dh[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  stream_chunks<Src, KS>(a, tl, [&](f32x4 (&acc)[4], const lds_f* b, int c, const typename Src::Side& sd) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const auto k = Src::cand(a, c, 16 * t + 4 * tl.lq + r, sd);
        acc[t][r] = Src::takes(a, k, y) ? g * Src::prob(k, y, acc[t][r], l_t) : 0.f;
      }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const lds_f* er = b + (16 * t + 4 * tl.lq + r) * kRS + tl.li;
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) dh[cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[t][r], er[16 * cc], dh[cc], 0, 0, 0);
      }
  });
  // dh[cc] register r of lane l: token 16 w + 4 lq + r of the tile, column 16 cc + li
#pragma unroll
  for (int cc = 0; cc < NC; ++cc)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int tk = tl.tok0 + 16 * tl.w + 4 * tl.lq + r, col = 16 * cc + tl.li;
      if (tk < tl.count && col < a.d_item) dh_part[((int64_t)blockIdx.y * a.T + tk) * a.d_item + col] = dh[cc][r];
    }
}

// the split partials in split order -> d_hidden; gpos != null (sampled): then the target's own term g_t+ E[y_t]
__global__ void __launch_bounds__(256) xent_dh_reduce_kernel(const XentArgs a, const float* __restrict__ dh_part,
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
  if (gpos != nullptr) s = fmaf(gpos[p], a.table[(int64_t)clamp_id(a.targets[p], a.n_items) * di + col], s);
  d_hidden[(int64_t)p * a.d_out + col] = s;
}

// ---- dE ---------------------------------------------------------------------------------------------------------------------
// A workgroup owns 64 rows of the dE grid (items / slots; a wave 16: their table rows stay in registers) and walks its token
// tiles in order.  The logit tile is formed untransposed, s(token 4 lq + r, row li), so that as the A operand of P^T H it is
// k-step r with k = token 4 lq + r; the B operand H(token, column) comes from the staged token tile.
template <class Src, int KS, int NC>
__device__ __forceinline__ void xent_de_body(const XentArgs& a, const float* __restrict__ lse,
                                             const float* __restrict__ d_loss, float* __restrict__ out) {
  __shared__ float sh[kTok * kRS];
  __shared__ float sl[kTok], sg[kTok];
  __shared__ int sy[kTok];
  const int count = a.count[0];
  const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4, w = threadIdx.x >> 6;
  const int di = a.d_item;
  const int row0 = blockIdx.x * kItems + 16 * w;
  const auto own = Src::owner(a, row0 + li);                       // this lane's row in the logit tiles
  float ef[KS];
  {
    const int64_t row = Src::table_row(a, own);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + lq;
      ef[s] = (row >= 0 && k < di) ? a.table[row * di + k] : 0.f;
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
  int tt0, tt1;
  Src::tile_range(a, (count + kTok - 1) / kTok, tt0, tt1);
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
    // logits: acc[j] register r of lane l = s(token 16 j + 4 lq + r, this lane's row)
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
        acc[j][r] = Src::takes(a, own, sy[q]) ? sg[q] * Src::prob(own, sy[q], acc[j][r], sl[q]) : 0.f;
      }
    // dE(row 4 lq' + r', column) += sum over tokens: D row = the row of A's lane (li), k = token, B = H(token, 16 cc + li)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const lds_f* hr = H + (16 * j + 4 * lq + r) * kRS + li;
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) de[cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[j][r], hr[16 * cc], de[cc], 0, 0, 0);
      }
  }
  // de[cc] register r of lane l: row (block, wave) 4 lq + r, column 16 cc + li; stored even for an empty token range
#pragma unroll
  for (int cc = 0; cc < NC; ++cc)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * cc + li < di) Src::store(a, out, row0 + 4 * lq + r, 16 * cc + li, de[cc][r]);
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

// What the four launchers start with: the argument and workspace-size checks (ptrs_ok: the caller's own pointers and K),
// the workspace layout, the token list and the kernels' common arguments.  A forward passes token_loss and lse (zeroed at
// every position), a backward d_hidden (zeroed).
int xent_begin(const srfrd_layout* lay, bool ptrs_ok, const float* table, const float* hidden, const int64_t* targets, int B,
               int L, int K, float* token_loss, float* lse, float* d_hidden, float* ws, int64_t ws_floats, hipStream_t st,
               XentWs& w, XentArgs& a) {
  if (int rc = check_layout(lay)) return rc;
  if (!ptrs_ok || !table || !hidden || !targets || !ws || B <= 0 || L <= 0) return SRFRD_E_ARG;
  w = xent_ws(*lay, B, L, K);
  if (ws_floats < w.total) return SRFRD_E_ARG;
  const int64_t T = (int64_t)B * L;
  hipLaunchKernelGGL(xent_count_kernel, dim3(w.nb_count), dim3(kCountBlock), 0, st, targets, T, (int*)(ws + w.cnt));
  hipLaunchKernelGGL(xent_compact_kernel, dim3(w.nb_count), dim3(kCountBlock), 0, st, targets, T, (const int*)(ws + w.cnt),
                     w.nb_count, (int*)(ws + w.idx), ws + w.tgt, (int*)(ws + w.count), token_loss, lse);
  if (int rc = (int)hipGetLastError()) return rc;
  if (d_hidden != nullptr)
    if (int rc = zero_floats(d_hidden, T * lay->d_out, st)) return rc;
  a = XentArgs{table, hidden, targets, (const int*)(ws + w.idx), (const int*)(ws + w.count), lay->d_item, lay->d_out,
               lay->n_items, w.S, w.n_chunks, (int)T, 0, nullptr, nullptr, K, w.St, 0};
  return 0;
}

}  // namespace
}  // namespace srfrd
