// Losses with K negatives per position: sampled softmax with per-position negatives, and BCE with K negatives generalised
// to gBCE (gSASRec, Petrov & Macdonald, RecSys 2023).  Both need the same logits: s_t+ = <h_t[:d_item], E[y_t]> and, for slot
// k of position t, s_tk = <h_t[:d_item], E[n_tk]>.  With K = 1 and beta = 1 the gbce objective is the reference's loss
// (trainer.py:36-38).  Tokens are the positions with targets != 0; a slot takes part when n_tk != 0 and, with remove_hits,
// n_tk != y_t.
//   softmax   loss_t = logsumexp({s_t+} u {s_tk - log_q[t, k]}) - s_t+
//   gbce      loss_t = beta softplus(-s_t+) + sum_k softplus(s_tk)
//
// Unlike the two softmax losses of srfrd_xent_common.h no table row is shared between tokens, so there is nothing for the
// matrix cores: a token's logits are 1 + K gathered rows against one hidden row.  A wave owns a position and keeps its
// hidden row in registers.  Its 64 lanes are four groups of 16; a group reads one table row per step, lane l of the group
// the columns VEC (16 j + l) + (0..VEC-1), j < NJ, so that adjacent lanes read adjacent 4 VEC bytes of the row (VEC = 4, 2
// or 1: the widest vector every row start is aligned for), and the dot product is reduced over the group by four DPP adds.
// kTnU such steps are issued together (16 rows of the wave in flight) with the ids of the next 16 slots already loading: the
// id -> row dependency is the latency to hide.  Slot 0 of this loop is the target, slot 1 + k negative k.
//
//   forward   tneg_fwd_kernel     per wave: the 1 + K logits; lanes 0..3 of each group take one logit each of the 16 (the
//                                 transcendentals run once per 16 slots, not once per 4) and keep an online (max, sum of exp)
//                                 or a softplus sum; merged in a fixed lane order -> token_loss, lse, block {sum, count}
//             tneg_stats_kernel   the block sums in block order -> stats {sum, count}
//   backward  tneg_bwd_kernel     the logits again (same code, same bits); g_tk per slot; dH += g_tk E[n_tk] in the lanes
//                                 that hold the row, the four groups added in group order -> d_hidden (the whole row, zeros
//                                 past d_item and at ignored positions); g_tk and its key to the contribution list
//   table     rank1_segment_kernel / rank1_merge_kernel   (srfrd_table_reduce_rank1, srfrd_table_reduce_mixed) below
// No float atomics anywhere: two identical calls are bitwise identical.

#include <climits>
#include <cmath>

#include "srfrd_xent_common.h"

namespace srfrd {
namespace {

constexpr int kTnWaves = 4;                  // positions per 256-thread workgroup (a wave each)
constexpr int kTnU = 4;                      // rows a lane group has in flight
constexpr int kTnChunk = 4 * kTnU;           // slots per step of a wave
constexpr int kSeg = SRFRD_TNEG_SPLIT_ROWS;  // sorted contribution rows per wave of the rank-1 reduce

struct TnegArgs {
  const float* table;
  const float* hidden;
  const int64_t* targets;
  const int64_t* neg;
  const float* log_q;   // may be null
  int d_item, d_out, n_items, K, T, objective, remove_hits;
  float beta;
};

struct TnegWs {
  int64_t part, bsum, bcnt, total;
  int nb;
};
inline int64_t rank1_part_floats(int64_t n, int d_item) { return a64(((n + kSeg - 1) / kSeg) * 2 * d_item); }
inline TnegWs tneg_ws(const srfrd_layout& ly, int B, int L, int K) {
  TnegWs w;
  const int64_t T = (int64_t)B * L;
  w.nb = (int)((T + kTnWaves - 1) / kTnWaves);
  int64_t o = 0;
  w.part = o; o += rank1_part_floats(T * (1 + (int64_t)K), ly.d_item);   // first: srfrd_table_reduce_rank1 finds it alone
  w.bsum = o; o += a64(w.nb);
  w.bcnt = o; o += a64(w.nb);
  w.total = o;
  return w;
}

// sum over the 16 lanes of a DPP row; every lane of the row ends with the same bits
__device__ __forceinline__ float row16_sum(float v) {
  v = quad_sum(v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));  // row_mirror
  return v;
}

template <int VEC> __device__ __forceinline__ void load_vec(float (&o)[VEC], const float* __restrict__ p);
template <> __device__ __forceinline__ void load_vec<1>(float (&o)[1], const float* __restrict__ p) { o[0] = p[0]; }
template <> __device__ __forceinline__ void load_vec<2>(float (&o)[2], const float* __restrict__ p) {
  const float2 v = *reinterpret_cast<const float2*>(p);
  o[0] = v.x; o[1] = v.y;
}
template <> __device__ __forceinline__ void load_vec<4>(float (&o)[4], const float* __restrict__ p) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}

// overflow-safe forms
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(__expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_f(float x) {
  const float e = __expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  return x >= 0.f ? r : e * r;
}

// A wave's view of its position p: the hidden row as this lane's columns, and the walk over the 1 + K slots in steps of
// kTnChunk.  Lane group g = lane / 16 takes slots c0 + 4 u + g, u < kTnU, of the step that starts at slot c0.
template <int VEC, int NJ>
struct TnegWalk {
  const TnegArgs& a;
  int64_t p;
  int y, lane, g, l16;
  int coff[NJ];           // first column of this lane's j-th vector, or -1 past d_item
  float h[NJ][VEC];
  int nid[kTnU];          // ids of the next step (0: takes no part)

  __device__ __forceinline__ TnegWalk(const TnegArgs& a_, int64_t p_, int y_) : a(a_), p(p_), y(y_) {
    lane = threadIdx.x & 63; g = lane >> 4; l16 = lane & 15;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = (16 * j + l16) * VEC;
      coff[j] = c < a.d_item ? c : -1;
#pragma unroll
      for (int k = 0; k < VEC; ++k) h[j][k] = coff[j] >= 0 ? a.hidden[p * a.d_out + c + k] : 0.f;
    }
    ids(0);
  }
  // the item of slot s as the loss sees it: the target for s = 0, negative s - 1 if it takes part, else 0
  __device__ __forceinline__ void ids(int c0) {
#pragma unroll
    for (int u = 0; u < kTnU; ++u) {
      const int s = c0 + 4 * u + g;
      int id = 0;
      if (s == 0) id = y;
      else if (s <= a.K) {
        id = clamp_id(a.neg[p * a.K + (s - 1)], a.n_items);
        if (a.remove_hits && id == y) id = 0;
      }
      nid[u] = id;
    }
  }
  // use(c0, id, x, v): the logits x[u] (every lane of the group holds them), ids and row fragments of one step
  template <class F>
  __device__ __forceinline__ void run(F&& use) {
    for (int c0 = 0; c0 <= a.K; c0 += kTnChunk) {
      int id[kTnU];
#pragma unroll
      for (int u = 0; u < kTnU; ++u) id[u] = nid[u];
      if (c0 + kTnChunk <= a.K) ids(c0 + kTnChunk);
      float v[kTnU][NJ][VEC], lq[kTnU], x[kTnU];
#pragma unroll
      for (int u = 0; u < kTnU; ++u) {
        const float* row = a.table + (int64_t)id[u] * a.d_item;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (id[u] != 0 && coff[j] >= 0) load_vec<VEC>(v[u][j], row + coff[j]);
          else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[u][j][k] = 0.f;
          }
        }
        const int s = c0 + 4 * u + g;
        lq[u] = (a.log_q != nullptr && id[u] != 0 && s >= 1) ? a.log_q[p * a.K + (s - 1)] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kTnU; ++u) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int k = 0; k < VEC; ++k) d = fmaf(h[j][k], v[u][j][k], d);
        x[u] = row16_sum(d) - lq[u];
      }
      use(c0, id, x, v);
    }
  }
};

template <int VEC, int NJ>
__global__ void __launch_bounds__(64 * kTnWaves) tneg_fwd_kernel(const TnegArgs a, float* __restrict__ token_loss,
                                                                 float* __restrict__ lse, float* __restrict__ bsum,
                                                                 float* __restrict__ bcnt) {
  __shared__ float s_loss[kTnWaves], s_cnt[kTnWaves];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * kTnWaves + w;
  const int64_t yr = p < a.T ? a.targets[p] : 0;
  float loss = 0.f, l = 0.f;
  if (yr != 0) {
    TnegWalk<VEC, NJ> wk(a, p, clamp_id(yr, a.n_items));
    const bool gbce = a.objective == SRFRD_TNEG_GBCE;
    float m = -INFINITY, sum = 0.f, sp = 0.f;           // softmax: online (m, sum); gbce: sum of softplus terms
    wk.run([&](int c0, const int (&id)[kTnU], const float (&x)[kTnU], const float (&)[kTnU][NJ][VEC]) {
      // lane u < kTnU of a group takes the group's slot c0 + 4 u + g
      float xs = 0.f;
      int ids = 0;
#pragma unroll
      for (int u = 0; u < kTnU; ++u)
        if (wk.l16 == u) { xs = x[u]; ids = id[u]; }
      if (wk.l16 < kTnU && ids != 0) {
        const bool tgt = c0 == 0 && lane == 0;
        if (tgt) sp = xs;
        if (gbce) sum += tgt ? a.beta * softplus_f(-xs) : softplus_f(xs);
        else online(m, sum, xs);
      }
    });
    // the lanes that hold terms: l16 < 4 of every group; lane 0 ends with all of them, in a fixed order
    if (gbce) {
      sum += __shfl_xor(sum, 1, 64); sum += __shfl_xor(sum, 2, 64);
      sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
      loss = sum;
    } else {
      constexpr int kSteps[4] = {1, 2, 16, 32};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float m2 = __shfl_xor(m, kSteps[i], 64), s2 = __shfl_xor(sum, kSteps[i], 64);
        merge(m, sum, m2, s2);
      }
      l = m + __logf(sum);
      loss = l - sp;
    }
  }
  if (lane == 0) {
    if (p < a.T) { token_loss[p] = loss; lse[p] = l; }
    s_loss[w] = loss;
    s_cnt[w] = yr != 0 ? 1.f : 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f, c = 0.f;
    for (int i = 0; i < kTnWaves; ++i) { t += s_loss[i]; c += s_cnt[i]; }
    bsum[blockIdx.x] = t;
    bcnt[blockIdx.x] = c;
  }
}

__global__ void __launch_bounds__(256) tneg_stats_kernel(const float* __restrict__ bsum, const float* __restrict__ bcnt, int nb,
                                                         float* __restrict__ stats) {
  __shared__ float sw[2][4];
  float t = 0.f, c = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) { t += bsum[i]; c += bcnt[i]; }
  t = wave_sum(t);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) { sw[0][threadIdx.x >> 6] = t; sw[1][threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    stats[0] = (sw[0][0] + sw[0][1]) + (sw[0][2] + sw[0][3]);
    stats[1] = (sw[1][0] + sw[1][1]) + (sw[1][2] + sw[1][3]);
  }
}

template <int VEC, int NJ>
__global__ void __launch_bounds__(64 * kTnWaves) tneg_bwd_kernel(const TnegArgs a, const float* __restrict__ lse,
                                                                 const float* __restrict__ d_loss, float* __restrict__ d_hidden,
                                                                 float* __restrict__ coef, int64_t* __restrict__ keys) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * kTnWaves + w;
  if (p >= a.T) return;
  const int64_t yr = a.targets[p];
  const int64_t r0 = p * (1 + (int64_t)a.K);
  float* dh_row = d_hidden + p * a.d_out;
  if (yr == 0) {
    for (int c = lane; c < a.d_out; c += 64) dh_row[c] = 0.f;
    for (int s = lane; s <= a.K; s += 64) { coef[r0 + s] = 0.f; keys[r0 + s] = 0; }
    return;
  }
  TnegWalk<VEC, NJ> wk(a, p, clamp_id(yr, a.n_items));
  const bool gbce = a.objective == SRFRD_TNEG_GBCE;
  const float l = lse[p], d = d_loss[p];
  float dh[NJ][VEC];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int k = 0; k < VEC; ++k) dh[j][k] = 0.f;
  wk.run([&](int c0, const int (&id)[kTnU], const float (&x)[kTnU], const float (&v)[kTnU][NJ][VEC]) {
    float cs = 0.f;
    int ids = 0;
#pragma unroll
    for (int u = 0; u < kTnU; ++u) {
      const bool tgt = c0 == 0 && u == 0 && wk.g == 0;
      float c = 0.f;
      if (id[u] != 0) {
        if (gbce) c = tgt ? -d * a.beta * sigmoid_f(-x[u]) : d * sigmoid_f(x[u]);
        else c = d * (__expf(x[u] - l) - (tgt ? 1.f : 0.f));
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < VEC; ++k) dh[j][k] = fmaf(c, v[u][j][k], dh[j][k]);
      if (wk.l16 == u) { cs = c; ids = id[u]; }
    }
    const int s = c0 + 4 * wk.l16 + wk.g;
    if (wk.l16 < kTnU && s <= a.K) { coef[r0 + s] = cs; keys[r0 + s] = ids; }
  });
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float t = dh[j][k];
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      if (wk.g == 0 && wk.coff[j] >= 0) dh_row[wk.coff[j] + k] = t;
    }
  for (int c = a.d_item + lane; c < a.d_out; c += 64) dh_row[c] = 0.f;
}

// ---- srfrd_table_reduce_rank1 ------------------------------------------------------------------------------------------------
// The sorted contribution list is cut into segments of kSeg rows, a wave each (lane = column): every wave does the same
// work however long the runs of equal keys are.  A run that lies inside one segment is summed and stored by that wave.  A
// run that crosses segment boundaries leaves one partial per segment it touches - part[seg][0] where it came in from the
// segment before, part[seg][1] where it starts in this segment and leaves it - and rank1_merge_kernel, in the wave of the
// segment the run starts in, adds them in segment order.  The cut depends on the sorted keys alone, so the order of every
// sum is fixed.  A segment whose last key is 0 lies inside the pad run at the front and is left after one load.
__device__ __forceinline__ void rank1_put(float* __restrict__ dst, int di, int lane, float acc) {
  if (lane < di) dst[lane] = acc;
}

// kMixed (srfrd_table_reduce_mixed): list entries o < n_rows are full rows, rows[o, :di], entering as fmaf(1, row, acc);
// entry o >= n_rows is the rank-1 row r = o - n_rows.  A lane carries its entry's source as one int for the readlane:
// the token of a rank-1 row, or ~o of a full row.
template <bool kMixed>
__global__ void __launch_bounds__(256) rank1_segment_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ order,
                                                            const float* __restrict__ rows, int64_t n_rows,
                                                            const float* __restrict__ coef, const float* __restrict__ hidden,
                                                            int d_out, int rpt, int64_t n, int di, float* __restrict__ grad_table,
                                                            float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t s0 = w * kSeg;
  if (s0 >= n) return;
  const int64_t s1 = s0 + kSeg < n ? s0 + kSeg : n;
  if (keys[s1 - 1] <= 0) return;
  const bool cont = s0 > 0 && keys[s0 - 1] == keys[s0];      // the first run came in from the segment before
  bool first = true;
  int64_t cur = keys[s0];
  float acc = 0.f;
  for (int64_t b = s0; b < s1; b += 64) {
    const int64_t i = b + lane;
    int64_t k = 0;
    int tok = 0;
    float c = 0.f;
    if constexpr (kMixed) {
      // (a lane past the segment takes the source of the segment's last entry: a valid row, not used)
      const int64_t o = order[i < s1 ? i : s1 - 1];
      float co = 1.f;
      if (o < n_rows) tok = ~(int)o;
      else {
        co = coef[o - n_rows];
        tok = (int)((o - n_rows) / rpt);
      }
      if (i < s1) { k = keys[i]; c = co; }
    } else if (i < s1) {
      k = keys[i];
      const int64_t o = order[i];
      c = coef[o];
      tok = (int)(o / rpt);
    }
    const int nb = (int)(s1 - b < 64 ? s1 - b : 64);
    for (int j0 = 0; j0 < nb; j0 += 8) {
      float hv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {                           // lanes past the segment hold token 0: a valid row, not used
        const int tq = __builtin_amdgcn_readlane(tok, j0 + q);
        const float* src = kMixed && tq < 0 ? rows + (int64_t)~tq * di : hidden + (int64_t)tq * d_out;
        hv[q] = lane < di ? src[lane] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (j0 + q < nb) {
          const int64_t kq = ((int64_t)__builtin_amdgcn_readlane((int)(k >> 32), j0 + q) << 32) |
                             (uint32_t)__builtin_amdgcn_readlane((int)k, j0 + q);
          const float cq = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c), j0 + q));
          if (kq != cur) {
            if (cur > 0) rank1_put(first && cont ? part + (w * 2) * di : grad_table + cur * di, di, lane, acc);
            cur = kq; acc = 0.f; first = false;
          }
          acc = fmaf(cq, hv[q], acc);
        }
      }
    }
  }
  if (cur <= 0) return;
  const bool goes_on = s1 < n && keys[s1] == cur;
  float* dst = grad_table + cur * di;
  if (first && cont) dst = part + (w * 2) * di;
  else if (goes_on) dst = part + (w * 2 + 1) * di;
  rank1_put(dst, di, lane, acc);
}

__global__ void __launch_bounds__(256) rank1_merge_kernel(const int64_t* __restrict__ keys, int64_t n, int di,
                                                          const float* __restrict__ part, float* __restrict__ grad_table) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t s0 = w * kSeg, s1 = s0 + kSeg;
  if (s1 >= n) return;
  const int64_t key = keys[s1 - 1];
  if (key <= 0 || keys[s1] != key) return;                       // no run leaves this segment
  if (s0 > 0 && keys[s0] == key && keys[s0 - 1] == key) return;  // it only passes through: its first segment sums it
  if (lane >= di) return;
  float acc = part[(w * 2 + 1) * di + lane];
  for (int64_t v = w + 1;; ++v) {
    acc += part[(v * 2) * di + lane];
    const int64_t e = (v + 1) * kSeg;
    if (e >= n || keys[e] != key) break;
  }
  grad_table[key * di + lane] = acc;
}

// (VEC, NJ) of a row width: the widest vector every row start of `table` is aligned for
template <class F>
void with_shape(int d_item, const float* table, F&& f) {
  const uintptr_t ad = (uintptr_t)table;
  if (d_item % 4 == 0 && ad % 16 == 0) return f(std::integral_constant<int, 4>(), std::integral_constant<int, 1>());
  if (d_item % 2 == 0 && ad % 8 == 0) {
    if (d_item <= 32) return f(std::integral_constant<int, 2>(), std::integral_constant<int, 1>());
    return f(std::integral_constant<int, 2>(), std::integral_constant<int, 2>());
  }
  switch ((d_item + 15) / 16) {
    case 1: return f(std::integral_constant<int, 1>(), std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 1>(), std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 1>(), std::integral_constant<int, 3>());
    default: return f(std::integral_constant<int, 1>(), std::integral_constant<int, 4>());
  }
}

// the checks every entry point starts with; 0 or the code to return
int tneg_check(const srfrd_layout* lay, int B, int L, int K, int objective, double beta, const float* log_q) {
  if (int rc = check_layout(lay)) return rc;
  if (B <= 0 || L <= 0 || K <= 0 || (int64_t)B * L * (1 + (int64_t)K) > INT_MAX) return SRFRD_E_ARG;
  if (objective != SRFRD_TNEG_SOFTMAX && objective != SRFRD_TNEG_GBCE) return SRFRD_E_ARG;
  if (objective == SRFRD_TNEG_GBCE) {
    if (log_q != nullptr || !(beta >= 0.0) || std::isinf(beta)) return SRFRD_E_ARG;
    if (lay->kind == SRFRD_SRFRN) return SRFRD_E_UNSUPPORTED;   // its logits include the fake slice: not built
  }
  return 0;
}

TnegArgs tneg_args(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                   const int64_t* negatives, const float* log_q, int K, int objective, double beta, int remove_hits, int B,
                   int L) {
  return TnegArgs{table, hidden, targets, negatives, log_q, lay->d_item, lay->d_out, lay->n_items, K, B * L, objective,
                  remove_hits ? 1 : 0, (float)beta};
}

}  // namespace
}  // namespace srfrd

using namespace srfrd;

extern "C" int64_t srfrd_tneg_workspace_floats(const srfrd_layout* lay, int B, int L, int K) {
  if (tneg_check(lay, B, L, K, SRFRD_TNEG_SOFTMAX, 1.0, nullptr) != 0) return 0;
  return tneg_ws(*lay, B, L, K).total;
}

extern "C" int srfrd_tneg_fwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                              const int64_t* negatives, const float* log_q, int K, int objective, double beta, int remove_hits,
                              int B, int L, float* token_loss, float* lse, float* stats, float* workspace, int64_t ws_floats,
                              void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = tneg_check(lay, B, L, K, objective, beta, log_q)) return rc;
  if (!table || !hidden || !targets || !negatives || !token_loss || !lse || !stats || !workspace) return SRFRD_E_ARG;
  const TnegWs w = tneg_ws(*lay, B, L, K);
  if (ws_floats < w.total) return SRFRD_E_ARG;
  const TnegArgs a = tneg_args(lay, table, hidden, targets, negatives, log_q, K, objective, beta, remove_hits, B, L);
  with_shape(lay->d_item, table, [&](auto vec, auto nj) {
    hipLaunchKernelGGL((tneg_fwd_kernel<decltype(vec)::value, decltype(nj)::value>), dim3(w.nb), dim3(64 * kTnWaves), 0, st, a,
                       token_loss, lse, workspace + w.bsum, workspace + w.bcnt);
  });
  hipLaunchKernelGGL(tneg_stats_kernel, dim3(1), dim3(256), 0, st, workspace + w.bsum, workspace + w.bcnt, w.nb, stats);
  return (int)hipGetLastError();
}

extern "C" int srfrd_tneg_bwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                              const int64_t* negatives, const float* log_q, int K, int objective, double beta, int remove_hits,
                              const float* lse, const float* d_token_loss, int B, int L, float* d_hidden, float* contrib_coef,
                              int64_t* contrib_keys, float* workspace, int64_t ws_floats, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = tneg_check(lay, B, L, K, objective, beta, log_q)) return rc;
  if (!table || !hidden || !targets || !negatives || !lse || !d_token_loss || !d_hidden || !contrib_coef || !contrib_keys ||
      !workspace)
    return SRFRD_E_ARG;
  const TnegWs w = tneg_ws(*lay, B, L, K);
  if (ws_floats < w.total) return SRFRD_E_ARG;
  const TnegArgs a = tneg_args(lay, table, hidden, targets, negatives, log_q, K, objective, beta, remove_hits, B, L);
  with_shape(lay->d_item, table, [&](auto vec, auto nj) {
    hipLaunchKernelGGL((tneg_bwd_kernel<decltype(vec)::value, decltype(nj)::value>), dim3(w.nb), dim3(64 * kTnWaves), 0, st, a,
                       lse, d_token_loss, d_hidden, contrib_coef, contrib_keys);
  });
  return (int)hipGetLastError();
}

extern "C" int srfrd_table_reduce_rank1(const int64_t* sorted_keys, const int64_t* order, const float* contrib_coef,
                                        const float* hidden, int d_out, int rows_per_token, int64_t n, int d_item,
                                        float* grad_table, float* workspace, int64_t ws_floats, void* stream) {
  if (!sorted_keys || !order || !contrib_coef || !hidden || !grad_table || !workspace || n <= 0 || n > INT_MAX ||
      rows_per_token < 1 || d_item < 1 || d_item > SRFRD_MAX_D || d_out < d_item)
    return SRFRD_E_ARG;
  if (ws_floats < rank1_part_floats(n, d_item)) return SRFRD_E_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)(((n + kSeg - 1) / kSeg + 3) / 4);
  hipLaunchKernelGGL(rank1_segment_kernel<false>, dim3(grid), dim3(256), 0, st, sorted_keys, order, (const float*)nullptr,
                     (int64_t)0, contrib_coef, hidden, d_out, rows_per_token, n, d_item, grad_table, workspace);
  hipLaunchKernelGGL(rank1_merge_kernel, dim3(grid), dim3(256), 0, st, sorted_keys, n, d_item, (const float*)workspace, grad_table);
  return (int)hipGetLastError();
}

static bool mixed_args_ok(int64_t n, int64_t n_rows, int rows_per_token, int d_item, int d_out) {
  return n > 0 && n <= INT_MAX && n_rows >= 0 && n_rows <= n && rows_per_token >= 1 && d_item >= 1 && d_item <= SRFRD_MAX_D &&
         d_out >= d_item;
}

extern "C" int64_t srfrd_table_reduce_mixed_workspace_floats(int64_t n, int d_item) {
  if (!mixed_args_ok(n, 0, 1, d_item, d_item)) return 0;
  return rank1_part_floats(n, d_item);
}

extern "C" int srfrd_table_reduce_mixed(const int64_t* sorted_keys, const int64_t* order, int64_t n, const float* rows,
                                        int64_t n_rows, const float* contrib_coef, const float* hidden, int d_out,
                                        int rows_per_token, int d_item, float* grad_table, float* workspace, int64_t ws_floats,
                                        void* stream) {
  if (!sorted_keys || !order || !grad_table || !workspace || !mixed_args_ok(n, n_rows, rows_per_token, d_item, d_out))
    return SRFRD_E_ARG;
  if ((n_rows > 0 && !rows) || (n > n_rows && (!contrib_coef || !hidden))) return SRFRD_E_ARG;
  if (ws_floats < rank1_part_floats(n, d_item)) return SRFRD_E_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)(((n + kSeg - 1) / kSeg + 3) / 4);
  hipLaunchKernelGGL(rank1_segment_kernel<true>, dim3(grid), dim3(256), 0, st, sorted_keys, order, rows, n_rows, contrib_coef,
                     hidden, d_out, rows_per_token, n, d_item, grad_table, workspace);
  hipLaunchKernelGGL(rank1_merge_kernel, dim3(grid), dim3(256), 0, st, sorted_keys, n, d_item, (const float*)workspace, grad_table);
  return (int)hipGetLastError();
}
