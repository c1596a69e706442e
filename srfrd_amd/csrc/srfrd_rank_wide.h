// Wide full-catalog top-k (include/srfrd_hip_topk_wide.h): exact lists of up to SRFRD_TOPK_WIDE_MAX items per user.  Included by
// srfrd_rank.hip behind its launchers: the kernels below are hooks over that file's stream templates (topk_stream,
// topk_stream16), so a score has the bits the k <= 64 ranking gives it, and the k <= 64 kernels are not touched.
//
//   A  group maxima.  Any partition of the rankable rows into groups works: a group maximum is a real score of a distinct
//      item, so the k-th largest group maximum is a lower bound on the k-th best score.  A catalog of 2 k stream chunks or
//      more keeps the chunk maxima (the existing topk_max*_kernel, as they are).  A smaller one needs finer groups: the lane
//      that owns four item rows of a 16-row tile keeps its own running maximum and stores it every 2^tshift tiles (stream16),
//      or once per chunk and wave (fp32 stream) - no cross-lane reduction, no change to the streams.
//   T  tau = k-th largest group maximum of the user: a radix select over the order-preserving key, one workgroup per user;
//      also resets the user's cursor (no memset: the call is one capturable chain of kernels).
//   B  the same stream again; scores >= tau go to the user's candidate list (kWideCap entries, atomic cursor).  The cursor
//      keeps counting past the capacity: a count above it is the user's overflow flag.
//   S  one workgroup per user sorts the candidates (value descending, id ascending) in LDS and writes the first k; with an
//      exclusion set, excluded candidates are dropped while the list is loaded.
//   F  one workgroup per OVERFLOWED user (every other one leaves at once) streams the item range by itself.
// A catalog with fewer than 2 k groups at the finest granularity has at most kWideCap rows: no maxima, tau = -inf, every
// finite score is a candidate.
#pragma once

#include "../../include/srfrd_hip_topk_wide.h"

namespace srfrd {

constexpr int kWideCap = 16384;          // candidates per user: 128 KiB of 8-byte keys, sorted in one workgroup's LDS
constexpr int kWideMax = SRFRD_TOPK_WIDE_MAX;
constexpr int kWideBlock = 1024;         // threads of the select and fallback workgroups

struct WideArgs {
  float* gmax;       // (B, gstride) group maxima (chunk path: the chunk maxima, = TopkArgs::cmax)
  int gstride;       // groups per user
  int gper;          // stream16, fine groups: groups per (chunk, lane quarter); 0: chunk maxima; -1: no maxima (tau = -inf)
  int tshift;        // stream16, fine groups: log2 of the 16-row tiles per group
  float* cmx;        // what the collection pass skips chunks by: (B, cstride) maxima per (chunk, lane quarter) that the threshold
  int cstride, cmul; // kernel folds the fine groups into (cmul 4), or the chunk maxima themselves (cmul 1: cmx = gmax)
  int cap;           // kWideCap
  int excl;          // an exclusion set is present (TopkArgs::xs / xoff)
};

// order-preserving 32-bit key of a float (larger float <=> larger key) and back
__device__ __forceinline__ uint32_t wide_okey(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float wide_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// a candidate as one 64-bit key whose ASCENDING order is (value descending, id ascending); -0 ranks as +0
constexpr unsigned long long kWideEmpty = ~0ull;
__device__ __forceinline__ unsigned long long wide_key(float v, int id) {
  return ((unsigned long long)(~wide_okey(v + 0.0f)) << 32) | (uint32_t)id;
}

// ---- pass A, fine groups ----------------------------------------------------------------------------------------------
template <int NU, bool SPLIT_E, bool EXCL>
__global__ void __launch_bounds__(kWaves16 * 64) wide_max16_kernel(const TopkArgs a, const WideArgs w) {
  const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
  const int tmask = (1 << w.tshift) - 1;
  float m[NU];
  topk_stream16<NU, SPLIT_E, EXCL>(a,
      [&](int n, int) { m[n] = -INFINITY; },
      [&](int n, int u0, int64_t item0, const f32x4& v) {
        m[n] = vmax3(vmax3(m[n], v[0], v[1]), v[2], v[3]);
        const int tile = (int)(item0 - a.item_lo) >> 4;          // 16-row tile of the range (chunks are whole tiles)
        if ((tile & tmask) == tmask) {                           // the group's last tile: its four-row strip of lane quarter lq
          if (u0 + li < a.B) w.gmax[(int64_t)(u0 + li) * w.gstride + ((tile >> w.tshift) << 2) + lq] = m[n];
          m[n] = -INFINITY;
        }
      },
      [&](int, int, int) {},
      [&](int, const int*) { return true; });
}

// fp32 stream: a lane's running maximum covers its rows of the wave's tiles of one chunk -> 4 groups per wave and chunk
template <bool EXCL>
__global__ void __launch_bounds__(512) wide_max_kernel(const TopkArgs a, const WideArgs w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, li = lane & 15, lq = lane >> 4;
  float m = -INFINITY;
  topk_stream<EXCL>(a,
      [&](int) { m = -INFINITY; },
      [&](int, int, int64_t, float v) { m = fmaxf(m, v); },
      [&](int u0, int chunk, lds_f*) {
        if (u0 + li < a.B) w.gmax[(int64_t)(u0 + li) * w.gstride + (chunk * nw + wave) * 4 + lq] = m;
      });
}

// ---- tau: k-th largest of the user's group maxima ------------------------------------------------------------------------
// Four 8-bit radix passes over the key, most significant digit first: a histogram of the keys that share the prefix found so
// far, then the digit whose bucket holds the k-th largest.  -inf is the smallest key a maximum can have, so a user with
// fewer than k finite maxima gets tau = -inf by the same walk.
__global__ void __launch_bounds__(256) wide_tau_kernel(const TopkArgs a, const WideArgs w) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_k;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = w.gper < 0 ? 0 : w.gstride;
  const float* row = w.gmax + (int64_t)b * w.gstride;
  float tau = -INFINITY;
  if (n >= a.k) {
    unsigned prefix = 0, kk = (unsigned)a.k;
    for (int shift = 24; shift >= 0; shift -= 8) {
      const unsigned himask = shift == 24 ? 0u : ~0u << (shift + 8);
      hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < n; i += 256) {
        const unsigned key = wide_okey(row[i]);
        if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        unsigned left = kk;
        int d = 255;
        for (; d > 0; --d) {
          if (hist[d] >= left) break;
          left -= hist[d];
        }
        s_prefix = prefix | ((unsigned)d << shift);
        s_k = left;
      }
      __syncthreads();
      prefix = s_prefix;
      kk = s_k;
    }
    tau = wide_unkey(prefix);
  }
  if (tid == 0) {
    a.tau[b] = tau;
    a.ccnt[b] = 0;
  }
  // stream16, fine groups: the maximum of every (chunk, lane quarter), one load per lane for the collection pass's skip test
  if (w.gper > 0 && w.cmul == 4)
    for (int c = tid; c < w.cstride; c += 256) {
      float m = -INFINITY;
      for (int j = 0; j < w.gper; ++j) m = fmaxf(m, row[((((c >> 2) * w.gper) + j) << 2) + (c & 3)]);
      w.cmx[(int64_t)b * w.cstride + c] = m;
    }
}

// ---- pass B ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wide_append(const TopkArgs& a, const WideArgs& w, int b, float v, int64_t item) {
  const int slot = atomicAdd(&a.ccnt[b], 1);                     // (counts on past the capacity: > cap flags the user)
  if (slot < w.cap) a.cand[(int64_t)b * w.cap + slot] = Cand{v, (int32_t)item};
}

template <int NU, bool SPLIT_E>
__global__ void __launch_bounds__(kWaves16 * 64) wide_collect16_kernel(const TopkArgs a, const WideArgs w) {
  const int li = threadIdx.x & 15, lq = (threadIdx.x & 63) >> 4;
  float tau[NU];
  topk_stream16<NU, SPLIT_E>(a,
      [&](int n, int u0) { tau[n] = u0 + li < a.B ? a.tau[u0 + li] : INFINITY; },
      [&](int n, int u0, int64_t item0, const f32x4& v) {
        if (!(vmax3(vmax3(v[0], v[1], v[2]), v[3], v[3]) >= tau[n])) return;
        unsigned hm = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) hm |= (v[e] != -INFINITY && v[e] >= tau[n]) ? 1u << e : 0u;
        while (hm) {
          const int e = __ffs(hm) - 1;
          hm &= hm - 1;
          const float ve = e == 0 ? v[0] : e == 1 ? v[1] : e == 2 ? v[2] : v[3];
          wide_append(a, w, u0 + li, ve, item0 + e);
        }
      },
      [&](int, int, int) {},
      // a chunk can hold a candidate of this lane's user only if the maximum of the lane's own groups of the chunk (or the
      // chunk's maximum) reaches tau; the wave skips a chunk no lane needs
      [&](int chunk, const int* u0s) {
        if (w.gper < 0) return true;
        bool hit = false;
#pragma unroll
        for (int n = 0; n < NU; ++n) {
          const int u = u0s[n] + li;
          if (u < a.B) hit |= w.cmx[(int64_t)u * w.cstride + chunk * w.cmul + (lq & (w.cmul - 1))] >= tau[n];
        }
        return __any(hit) != 0;
      });
}

__global__ void __launch_bounds__(512) wide_collect_kernel(const TopkArgs a, const WideArgs w) {
  const int li = threadIdx.x & 15;
  float tau = INFINITY;
  topk_stream(a,
      [&](int u0) { tau = u0 + li < a.B ? a.tau[u0 + li] : INFINITY; },
      [&](int u0, int c, int64_t item, float v) {
        if (v != -INFINITY && v >= tau) wide_append(a, w, u0 + c, v, item);
      },
      [&](int, int, lds_f*) {});
}

// ascending bitonic sort of P (a power of two) 64-bit keys in LDS by the whole workgroup
__device__ __forceinline__ void wide_sort(unsigned long long* sk, int P) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += nthr) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long x = sk[i], y = sk[ixj];
          if ((x > y) == ((i & k) == 0)) { sk[i] = y; sk[ixj] = x; }
        }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ void wide_write(const unsigned long long* sk, int n_sorted, int b, int k, int64_t* topk_idx,
                                           float* topk_val) {
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const unsigned long long key = i < n_sorted ? sk[i] : kWideEmpty;
    const bool ok = key != kWideEmpty;
    topk_idx[(int64_t)b * k + i] = ok ? (int64_t)(uint32_t)key : -1;
    topk_val[(int64_t)b * k + i] = ok ? wide_unkey(~(uint32_t)(key >> 32)) : -INFINITY;
  }
}

// ---- S: the user's candidates, sorted; the order the cursor handed out slots in does not reach the output ------------------
__global__ void __launch_bounds__(kWideBlock) wide_select_kernel(const TopkArgs a, const WideArgs w, int64_t* __restrict__ topk_idx,
                                                                 float* __restrict__ topk_val) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  unsigned long long* sk = (unsigned long long*)smem;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = a.ccnt[b];
  if (n > w.cap) return;                            // overflowed: the whole list is the fallback's
  int P = 2;
  while (P < n) P <<= 1;
  const Cand* c = a.cand + (int64_t)b * w.cap;
  for (int i = tid; i < P; i += kWideBlock) {
    unsigned long long key = kWideEmpty;
    if (i < n) {
      const Cand x = c[i];
      if (!(w.excl && excl_has(a, b, x.i))) key = wide_key(x.v, x.i);
    }
    sk[i] = key;
  }
  __syncthreads();
  wide_sort(sk, P);
  wide_write(sk, P, b, a.k, topk_idx, topk_val);
}

// ---- F: exact for any input.  The workgroup of an overflowed user scores 1024 rows at a time - one row per thread, one
// fp64 chain in channel order, rounded once: a row's value does not depend on where it sits, so bit-identical rows tie
// exactly - and keeps the best 1024 keys sorted in LDS.  Keys that beat the current k-th are appended behind them; when the
// next block's would not fit, the 2048 keys are sorted again.
// (the body, shared with the filtered form of srfrd_rank_filter.h: allowed(item) is one more test beside excl_has)
template <class ALLOWED>
__device__ __forceinline__ void wide_fallback_user(const TopkArgs& a, const WideArgs& w, int64_t* __restrict__ topk_idx,
                                                   float* __restrict__ topk_val, ALLOWED&& allowed) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ unsigned long long sk[2 * kWideBlock];
  __shared__ float sh[SRFRD_MAX_D];
  __shared__ double s_side;
  __shared__ int s_slot;
  const srfrd_layout& ly = a.ly;
  const int di = ly.d_item, dout = ly.d_out, D = ly.D;
  const float* hrow = a.hidden + ((int64_t)b * a.L + (a.L - 1)) * dout;
  if (tid < di) sh[tid] = hrow[tid];
  if (tid == 64) {
    double s = 0.0;
    if (ly.kind == SRFRD_SRFRN) {
      const int lab = clamp_id(a.user_label[b], 2);
      for (int c = di; c < D; ++c) s += (double)hrow[c] * (double)a.dense[ly.off_side + lab * ly.d_fake + (c - di)];
    }
    s_side = s;
    s_slot = 0;
  }
  sk[tid] = kWideEmpty;
  sk[kWideBlock + tid] = kWideEmpty;
  __syncthreads();
  const ItemTable table{ly.table_bf16 ? nullptr : (const float*)a.table, ly.table_bf16 ? (const uint16_t*)a.table : nullptr};
  unsigned long long kth = kWideEmpty;
  int fill = 0;                                     // appended keys behind the sorted 1024 (uniform)
  auto merge = [&]() {
    if (tid >= fill) sk[kWideBlock + tid] = kWideEmpty;
    __syncthreads();
    wide_sort(sk, 2 * kWideBlock);
    kth = sk[a.k - 1];
    fill = 0;
    if (tid == 0) s_slot = 0;
    __syncthreads();
  };
  for (int64_t r0 = a.item_lo; r0 < a.item_hi; r0 += kWideBlock) {
    const int64_t item = r0 + tid;
    bool ok = item < a.item_hi && !(a.exclude_pad && item == 0);
    if (ok && w.excl) ok = !excl_has(a, b, item);
    if (ok) ok = allowed(item);
    unsigned long long key = kWideEmpty;
    if (ok) {
      double s = 0.0;
      for (int c = 0; c < di; ++c) s += (double)sh[c] * (double)table(item * di + c);
      key = wide_key((float)(s + s_side), (int)item);
    }
    const bool q = key < kth;
    const int total = __syncthreads_count(q);
    if (total == 0) continue;
    if (fill + total > kWideBlock) merge();
    if (q) sk[kWideBlock + atomicAdd(&s_slot, 1)] = key;
    fill += total;
    __syncthreads();
  }
  merge();
  wide_write(sk, kWideBlock, b, a.k, topk_idx, topk_val);
}

__global__ void __launch_bounds__(kWideBlock) wide_fallback_kernel(const TopkArgs a, const WideArgs w, int64_t* __restrict__ topk_idx,
                                                                   float* __restrict__ topk_val) {
  if (a.ccnt[blockIdx.x] <= w.cap) return;
  wide_fallback_user(a, w, topk_idx, topk_val, [](int64_t) { return true; });
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
enum WidePath { kWideFine = 0, kWideChunk = 1, kWideAll = 2 };
enum WideKernel { kWideMax16 = 100, kWideMaxF32, kWideTau, kWideCollect16, kWideCollect, kWideSelect, kWideFallback };

struct WidePlan {
  int rc;
  RankPlan base;     // the k <= 64 plan of the same call: route, chunking, grids and LDS of the stream passes, refusals
  int path, groups, gper, tshift;
  int n_launches;
  RankLaunch launch[8];
};

static const RankLaunch* wide_find(const RankPlan& p, int k0, int k1) {
  for (int i = 0; i < p.n_launches; ++i)
    if (p.launch[i].kernel == k0 || p.launch[i].kernel == k1) return &p.launch[i];
  return nullptr;
}

// Rules.  (1) 2 k stream chunks or more: the chunk maxima.  (2) else the finest-needed groups: on stream16 the coarsest
// power-of-two split of a chunk's lane-quarter strips that gives 4 k groups (or the finest, 4 rows, if that gives 2 k); on
// the fp32 stream the 32 groups per chunk.  (3) else no maxima: fewer than 2 k groups of 4 (8) rows are at most
// 8 k (16 k) <= kWideCap rows, so every finite score fits the candidate list.
static WidePlan wide_plan(const srfrd_layout& lay, int B, int k, int64_t item_lo, int64_t item_hi, bool excl, int switches, int n_cu) {
  WidePlan p = {};
  p.base = rank_plan(lay, SRFRD_RANK_TOPK, B, k < 64 ? k : 64, item_lo, item_hi, excl, switches, n_cu);
  if (p.base.rc) { p.rc = p.base.rc; return p; }
  const RankPlan& r = p.base;
  const int64_t sc = r.stream_chunks;
  const RankLaunch* pa = wide_find(r, kTopkMax16, kTopkMax);
  const RankLaunch* pb = wide_find(r, kTopkCollect16, kTopkCollect);
  p.gper = -1;
  if (sc >= 2 * (int64_t)k) {
    p.path = kWideChunk; p.groups = (int)sc; p.gper = 0;
  } else if (r.stream16) {
    const int ntile = r.crows >> 4;
    int gper = 1;
    while (gper < ntile && sc * 4 * gper < 4 * (int64_t)k) gper <<= 1;
    if (sc * 4 * gper >= 2 * (int64_t)k) {
      p.path = kWideFine; p.groups = (int)(sc * 4 * gper); p.gper = gper;
      for (int t = ntile / gper; t > 1; t >>= 1) ++p.tshift;
    } else p.path = kWideAll;
  } else {
    if (sc * 32 >= 2 * (int64_t)k) { p.path = kWideFine; p.groups = (int)(sc * 32); p.gper = 1; }
    else p.path = kWideAll;
  }
  const auto add = [&](int kernel, int64_t g, int block, int64_t lds) { p.launch[p.n_launches++] = {kernel, (int)g, block, lds}; };
  if (excl) add(kExclPrep, B, 1024, 0);
  if (p.path == kWideChunk) add(pa->kernel, pa->grid, pa->block, pa->lds);
  else if (p.path == kWideFine) add(r.stream16 ? kWideMax16 : kWideMaxF32, pa->grid, pa->block, pa->lds);
  add(kWideTau, B, 256, 0);
  add(r.stream16 ? kWideCollect16 : kWideCollect, pb->grid, pb->block, pb->lds);
  add(kWideSelect, B, kWideBlock, (int64_t)kWideCap * 8);
  add(kWideFallback, B, kWideBlock, 0);
  return p;
}

static void wide_launch_name(const WidePlan& p, const RankLaunch& l, char* buf, int len) {
  const RankPlan& r = p.base;
  const char *se = r.split_e ? "true" : "false", *x = r.excl ? "true" : "false";
  switch (l.kernel) {
    case kWideMax16: snprintf(buf, len, "srfrd::wide_max16_kernel<%d,%s,%s>", r.nu, se, x); return;
    case kWideMaxF32: snprintf(buf, len, "srfrd::wide_max_kernel<%s>", x); return;
    case kWideTau: snprintf(buf, len, "srfrd::wide_tau_kernel"); return;
    case kWideCollect16: snprintf(buf, len, "srfrd::wide_collect16_kernel<%d,%s>", r.nu, se); return;
    case kWideCollect: snprintf(buf, len, "srfrd::wide_collect_kernel"); return;
    case kWideSelect: snprintf(buf, len, "srfrd::wide_select_kernel"); return;
    case kWideFallback: snprintf(buf, len, "srfrd::wide_fallback_kernel"); return;
    default: launch_name(r, l, buf, len);
  }
}

// workspace: [group maxima B * wide_gfloats f32][tau B f32][cursor B + 4 i32][candidates B * kWideCap][(chunk, lane
// quarter) maxima B * 4 ceil(n_rows / 256) f32]
// wide_gfloats: at least the groups of any plan of (k, n_rows) - chunk maxima: ceil(n_rows / 256) or fewer; fine groups on
// stream16: under 8 k (the coarsest split reaching 4 k) and at most 128 per 256 rows; on the fp32 stream 32 per chunk of a
// catalog under 2 k chunks
static int64_t wide_gfloats(int k, int64_t n_rows) {
  const int64_t nc = (n_rows + 255) / 256, fine = 128 * nc < 64 * (int64_t)k ? 128 * nc : 64 * (int64_t)k;
  return nc > fine ? nc : fine;
}
static int64_t wide_off(int B, int k, int64_t n_rows, int which) {
  const int64_t sizes[5] = {(int64_t)B * wide_gfloats(k, n_rows) * 4, (int64_t)B * 4, ((int64_t)B + 4) * 4,
                            (int64_t)B * kWideCap * (int64_t)sizeof(Cand), (int64_t)B * ((n_rows + 255) / 256) * 16};
  int64_t off = 0;
  for (int i = 0; i < which; ++i) off += (sizes[i] + 255) & ~255ll;
  return off;
}

}  // namespace srfrd

extern "C" int srfrd_topk_wide_plan(const srfrd_layout* lay, int B, int k, int64_t item_lo, int64_t item_hi, int excl, int switches,
                                    int n_cu, int max_launches, char* names, int name_len, int32_t* geom, int32_t* sizes) {
  if (!lay || B <= 0 || k < 1 || k > kWideMax || item_lo < 0 || item_hi <= item_lo || item_hi > (int64_t)lay->n_items + 1 ||
      n_cu <= 0 || max_launches < 0)
    return SRFRD_E_ARG;
  const WidePlan p = wide_plan(*lay, B, k, item_lo, item_hi, excl != 0, switches, n_cu);
  if (p.rc) return p.rc;
  for (int i = 0; i < p.n_launches && i < max_launches; ++i) {
    const RankLaunch& l = p.launch[i];
    if (names && name_len > 0) wide_launch_name(p, l, names + (int64_t)i * name_len, name_len);
    if (geom) { geom[3 * i] = l.grid; geom[3 * i + 1] = l.block; geom[3 * i + 2] = (int32_t)l.lds; }
  }
  if (sizes) { sizes[0] = p.path; sizes[1] = kWideCap; sizes[2] = p.groups; }
  return p.n_launches;
}

extern "C" int64_t srfrd_topk_wide_workspace_bytes(int B, int k, int64_t n_rows) {
  if (B <= 0 || k < 1 || k > kWideMax || n_rows <= 0) return 0;
  return wide_off(B, k, n_rows, 5);
}

extern "C" int srfrd_logits_topk_wide(const srfrd_layout* lay, const void* item_table, const float* dense, const float* hidden,
                                      int B, int L, int64_t item_lo, int64_t item_hi, int exclude_pad, const int64_t* user_label,
                                      int k, const int64_t* excl_ptr, const int32_t* excl_items, int max_row, int64_t* topk_idx,
                                      float* topk_val, void* workspace, int64_t ws_bytes, void* excl_workspace, void* stream) {
  if (!topk_idx || !topk_val || !workspace || k < 1 || k > kWideMax) return SRFRD_E_ARG;
  if (int rc = topk_args_check(lay, item_table, dense, hidden, B, L, item_lo, item_hi, user_label)) return rc;
  if (ws_bytes < srfrd_topk_wide_workspace_bytes(B, k, item_hi - item_lo)) return SRFRD_E_ARG;
  if (int rc = excl_args(excl_ptr, excl_items, max_row, excl_workspace, B, item_hi)) return rc;
  const WidePlan p = wide_plan(*lay, B, k, item_lo, item_hi, excl_ptr != nullptr, read_switches(), num_cu());
  if (p.rc) return p.rc;
  const int64_t n_rows = item_hi - item_lo;
  // wide_gfloats bounds the groups of every plan (see there); held here because a plan past it would write past the maxima
  if (p.groups > wide_gfloats(k, n_rows)) return SRFRD_E_DEVICE;
  const RankPlan& r = p.base;
  RankIO io = {excl_ptr, excl_items, max_row, topk_idx, topk_val};
  TopkArgs a = rank_args(r, lay, item_table, dense, hidden, B, L, item_lo, item_hi, exclude_pad, user_label, k, max_row,
                         excl_workspace, io);
  char* ws = (char*)workspace;
  WideArgs w = {};
  w.gmax = a.cmax = (float*)(ws + wide_off(B, k, n_rows, 0));
  a.tau = (float*)(ws + wide_off(B, k, n_rows, 1));
  a.ccnt = (int32_t*)(ws + wide_off(B, k, n_rows, 2));
  a.cand = (Cand*)(ws + wide_off(B, k, n_rows, 3));
  w.gstride = p.path == kWideAll ? 1 : p.groups;
  w.cmx = w.gmax; w.cstride = w.gstride; w.cmul = 1;
  if (p.path == kWideFine && r.stream16) { w.cmx = (float*)(ws + wide_off(B, k, n_rows, 4)); w.cstride = r.stream_chunks * 4; w.cmul = 4; }
  w.gper = p.gper; w.tshift = p.tshift; w.cap = kWideCap; w.excl = excl_ptr != nullptr;
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < p.n_launches; ++i) {
    const RankLaunch& l = p.launch[i];
    int rc = 0;
    switch (l.kernel) {
      case kWideMax16:
        rc = with_flag(r.excl, [&](auto x) { return with_stream16<decltype(x)::value>(r, [&](auto nu, auto se) {
          return launch_rank(wide_max16_kernel<decltype(nu)::value, decltype(se)::value, decltype(x)::value>, l, st, a, w); }); });
        break;
      case kWideMaxF32: rc = with_flag(r.excl, [&](auto x) { return launch_rank(wide_max_kernel<decltype(x)::value>, l, st, a, w); }); break;
      case kWideTau: rc = launch_rank(wide_tau_kernel, l, st, a, w); break;
      case kWideCollect16:
        rc = with_stream16<false>(r, [&](auto nu, auto se) {
          return launch_rank(wide_collect16_kernel<decltype(nu)::value, decltype(se)::value>, l, st, a, w); });
        break;
      case kWideCollect: rc = launch_rank(wide_collect_kernel, l, st, a, w); break;
      case kWideSelect: rc = launch_rank(wide_select_kernel, l, st, a, w, topk_idx, topk_val); break;
      case kWideFallback: rc = launch_rank(wide_fallback_kernel, l, st, a, w, topk_idx, topk_val); break;
      default: rc = launch_one(r, l, a, io, st);        // the exclusion pre-pass and the chunk maxima: the k <= 64 kernels
    }
    if (rc) return rc;
  }
  return 0;
}
