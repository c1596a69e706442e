// Item filters (include/srfrd_hip_filter.h): exact top-k and target rank over the items a packed bitmap allows.  Included by
// srfrd_rank.hip behind srfrd_rank_wide.h: the kernels below are one more family of hooks over the stream templates
// (topk_stream, topk_stream16) - the same scores with the same bits; a disallowed score turns to -inf inside elem, before it
// reaches a maximum, a candidate list or a count.  wide_tau_kernel and wide_select_kernel run as they are.
//
// The threshold is a BOUND here, not an expectation: groups of at most r rows with k r <= kWideCap (allow_rule).  Fewer than
// k finite maxima means fewer than k r allowed rows; otherwise every candidate lies in a group whose maximum reaches tau,
// which - ties of maxima at tau aside - are at most k groups.  Either way the list holds them, whatever the filter is.
#pragma once

#include "../../include/srfrd_hip_filter.h"

namespace srfrd {

struct AllowArgs {
  const uint32_t* words;   // (n_groups, wpg) packed rows over absolute item ids
  const int64_t* group;    // (B) bitmap row per user, or nullptr: row 0
  int n_groups;
  int last;                // the last word a two-word window may start at: srfrd_item_mask_words(n_items + 1) - 2
  int64_t wpg;
};

// the bitmap row of user u, read once per user tile (begin): the lane keeps the pointer
__device__ __forceinline__ const uint32_t* allow_row(const AllowArgs& f, int u, int B) {
  int64_t g = 0;
  if (f.group && u < B) {
    g = f.group[u];
    g = g < 0 ? 0 : g >= f.n_groups ? f.n_groups - 1 : g;
  }
  return f.words + g * f.wpg;
}
// bits e = 0..3: items item0 + e.  The four bits straddle a word when item_lo % 4 != 0: a two-word window, funnel-shifted (the
// shift is item0 & 31, never 32).  Rows past the catalog (a chunk's tail, already -inf) clamp to the row's zero words.
__device__ __forceinline__ unsigned allow_bits4(const uint32_t* row, int last, int64_t item0) {
  const int wi = min((int)(item0 >> 5), last);
  return __funnelshift_r(row[wi], row[wi + 1], (unsigned)item0 & 31u) & 15u;
}
__device__ __forceinline__ bool allow_bit(const uint32_t* row, int last, int64_t item) {
  const int wi = min((int)(item >> 5), last + 1);
  return ((row[wi] >> ((unsigned)item & 31u)) & 1u) != 0;
}
__device__ __forceinline__ f32x4 allow_mask4(const f32x4& v, unsigned bits) {
  f32x4 r;
  r[0] = (bits & 1u) ? v[0] : -INFINITY;
  r[1] = (bits & 2u) ? v[1] : -INFINITY;
  r[2] = (bits & 4u) ? v[2] : -INFINITY;
  r[3] = (bits & 8u) ? v[3] : -INFINITY;
  return r;
}

// ---- packing: a wave's ballot over 64 items is two words of the row ---------------------------------------------------------
__global__ void __launch_bounds__(256) item_mask_pack_kernel(const uint8_t* __restrict__ mask, int n_groups, int64_t n_rows,
                                                            int64_t W, uint32_t* __restrict__ words) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  for (int g = blockIdx.y; g < n_groups; g += gridDim.y) {
    const bool on = i < n_rows && mask[(int64_t)g * n_rows + i] != 0;
    const unsigned long long bal = __ballot(on);
    const int64_t wi = (i >> 5);
    if ((lane & 31) == 0 && wi < W) words[(int64_t)g * W + wi] = (uint32_t)(lane ? bal >> 32 : bal);
  }
}

// ---- group maxima -----------------------------------------------------------------------------------------------------------
// stream16 at one user tile per wave: wide_max16_kernel's strips (a lane quarter's four rows over 2^tshift tiles)
template <bool SPLIT_E, bool EXCL>
__global__ void __launch_bounds__(kWaves16 * 64) allow_max16_kernel(const TopkArgs a, const WideArgs w, const AllowArgs f) {
  const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
  const int tmask = (1 << w.tshift) - 1;
  float m = -INFINITY;
  const uint32_t* row = f.words;
  topk_stream16<1, SPLIT_E, EXCL>(a,
      [&](int, int u0) { m = -INFINITY; row = allow_row(f, u0 + li, a.B); },
      [&](int, int u0, int64_t item0, const f32x4& vin) {
        const f32x4 v = allow_mask4(vin, allow_bits4(row, f.last, item0));
        m = vmax3(vmax3(m, v[0], v[1]), v[2], v[3]);
        const int tile = (int)(item0 - a.item_lo) >> 4;
        if ((tile & tmask) == tmask) {
          if (u0 + li < a.B) w.gmax[(int64_t)(u0 + li) * w.gstride + ((tile >> w.tshift) << 2) + lq] = m;
          m = -INFINITY;
        }
      },
      [&](int, int, int) {},
      [&](int, const int*) { return true; });
}

// fp32 stream: wide_max_kernel's groups (the 8 rows a lane quarter of one wave owns of a chunk)
template <bool EXCL>
__global__ void __launch_bounds__(512) allow_max_kernel(const TopkArgs a, const WideArgs w, const AllowArgs f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, li = lane & 15, lq = lane >> 4;
  float m = -INFINITY;
  const uint32_t* row = f.words;
  topk_stream<EXCL>(a,
      [&](int u0) { m = -INFINITY; row = allow_row(f, u0 + li, a.B); },
      [&](int, int, int64_t item, float v) { m = fmaxf(m, allow_bit(row, f.last, item) ? v : -INFINITY); },
      [&](int u0, int chunk, lds_f*) {
        if (u0 + li < a.B) w.gmax[(int64_t)(u0 + li) * w.gstride + (chunk * nw + wave) * 4 + lq] = m;
      });
}

// ---- collection ---------------------------------------------------------------------------------------------------------------
template <bool SPLIT_E, bool EXCL>
__global__ void __launch_bounds__(kWaves16 * 64) allow_collect16_kernel(const TopkArgs a, const WideArgs w, const AllowArgs f) {
  const int li = threadIdx.x & 15, lq = (threadIdx.x & 63) >> 4;
  float tau = INFINITY;
  const uint32_t* row = f.words;
  topk_stream16<1, SPLIT_E, EXCL>(a,
      [&](int, int u0) { tau = u0 + li < a.B ? a.tau[u0 + li] : INFINITY; row = allow_row(f, u0 + li, a.B); },
      [&](int, int u0, int64_t item0, const f32x4& v) {
        if (!(vmax3(vmax3(v[0], v[1], v[2]), v[3], v[3]) >= tau)) return;          // (no allowed score is above the unmasked one)
        const unsigned bits = allow_bits4(row, f.last, item0);
        unsigned hm = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) hm |= (v[e] != -INFINITY && v[e] >= tau) ? 1u << e : 0u;
        hm &= bits;
        while (hm) {
          const int e = __ffs(hm) - 1;
          hm &= hm - 1;
          const float ve = e == 0 ? v[0] : e == 1 ? v[1] : e == 2 ? v[2] : v[3];
          wide_append(a, w, u0 + li, ve, item0 + e);
        }
      },
      [&](int, int, int) {},
      [&](int chunk, const int* u0s) {
        if (w.gper < 0) return true;
        const int u = u0s[0] + li;
        const bool hit = u < a.B && w.cmx[(int64_t)u * w.cstride + chunk * 4 + lq] >= tau;
        return __any(hit) != 0;
      });
}

template <bool EXCL>
__global__ void __launch_bounds__(512) allow_collect_kernel(const TopkArgs a, const WideArgs w, const AllowArgs f) {
  const int li = threadIdx.x & 15;
  float tau = INFINITY;
  const uint32_t* row = f.words;
  topk_stream<EXCL>(a,
      [&](int u0) { tau = u0 + li < a.B ? a.tau[u0 + li] : INFINITY; row = allow_row(f, u0 + li, a.B); },
      [&](int u0, int c, int64_t item, float v) {
        if (v != -INFINITY && v >= tau && allow_bit(row, f.last, item)) wide_append(a, w, u0 + c, v, item);
      },
      [&](int, int, lds_f*) {});
}

// ---- target rank: the count passes ----------------------------------------------------------------------------------------------
template <bool SPLIT_E, bool EXCL>
__global__ void __launch_bounds__(kWaves16 * 64) allow_count16_kernel(const TopkArgs a, const AllowArgs f) {
  const int lane = threadIdx.x & 63, li = lane & 15;
  float st = INFINITY;
  int cnt = 0;
  const uint32_t* row = f.words;
  topk_stream16<1, SPLIT_E, EXCL>(a,
      [&](int, int u0) { st = u0 + li < a.B ? a.tau[u0 + li] : INFINITY; cnt = 0; row = allow_row(f, u0 + li, a.B); },
      [&](int, int, int64_t item0, const f32x4& v) {
        const unsigned bits = allow_bits4(row, f.last, item0);
        const unsigned above = (v[0] > st ? 1u : 0u) | (v[1] > st ? 2u : 0u) | (v[2] > st ? 4u : 0u) | (v[3] > st ? 8u : 0u);
        cnt += __popc(above & bits);
      },
      [&](int, int, int) {},
      [&](int, const int*) { return true; });
  int c = cnt + __shfl_xor(cnt, 16, 64);
  c += __shfl_xor(c, 32, 64);
  const int group = blockIdx.x / a.wg_per_group, wave = threadIdx.x >> 6;        // (topk_stream16's user tiles at NU = 1)
  const int u = ((group * kWaves16 + wave) << 4) + li;
  if (lane < 16 && u < a.B && c) atomicAdd(&a.ccnt[u], c);
}

template <bool EXCL>
__global__ void __launch_bounds__(512) allow_count_kernel(const TopkArgs a, const AllowArgs f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, li = lane & 15;
  float st = INFINITY;
  int cnt = 0;
  const uint32_t* row = f.words;
  topk_stream<EXCL>(a,
      [&](int u0) { st = u0 + li < a.B ? a.tau[u0 + li] : INFINITY; cnt = 0; row = allow_row(f, u0 + li, a.B); },
      [&](int, int, int64_t item, float v) { cnt += (int)(v > st && allow_bit(row, f.last, item)); },
      [&](int u0, int, lds_f* sM) {
        int c = cnt + __shfl_xor(cnt, 16, 64);
        c += __shfl_xor(c, 32, 64);
        if (lane < 16) sM[wave * 16 + lane] = __int_as_float(c);
        __syncthreads();
        if (threadIdx.x < 16 && u0 + (int)threadIdx.x < a.B) {
          int tot = 0;
          for (int x = 0; x < nw; ++x) tot += __float_as_int(sM[x * 16 + threadIdx.x]);
          if (tot) atomicAdd(&a.ccnt[u0 + threadIdx.x], tot);
        }
      });
}

// ---- the fallback workgroup: wide_fallback_kernel's body with the bit tested beside excl_has ---------------------------------
__global__ void __launch_bounds__(kWideBlock) allow_fallback_kernel(const TopkArgs a, const WideArgs w, const AllowArgs f,
                                                                    int64_t* __restrict__ topk_idx, float* __restrict__ topk_val) {
  if (a.ccnt[blockIdx.x] <= w.cap) return;
  const uint32_t* row = allow_row(f, blockIdx.x, a.B);
  wide_fallback_user(a, w, topk_idx, topk_val, [&](int64_t item) { return allow_bit(row, f.last, item); });
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
enum AllowKernel { kAllowMax16 = 200, kAllowMaxF32, kAllowCollect16, kAllowCollect, kAllowFallback, kAllowCount16, kAllowCount };

struct AllowRule {
  int path;          // kWideFine / kWideAll
  int tshift;        // stream16: log2 of the 16-row tiles per group
  int gper;          // groups per (256-row chunk, lane quarter) on stream16, 1 on the fp32 stream; -1: no maxima
  int rows;          // rows of a group (0: no groups)
  int per_chunk;     // groups per 256-row chunk
};

// THE rule (host only; srfrd_topk_allow_plan reports it): groups of at most `rows` rows with rows * k <= kWideCap.
static AllowRule allow_rule(bool stream16, int k, int64_t n_rows) {
  AllowRule r = {kWideAll, 0, -1, 0, 0};
  if (n_rows <= kWideCap) return r;                  // every allowed finite score is a candidate
  r.path = kWideFine;
  if (stream16) {
    int t = 4;                                       // 16 tiles of a 256-row chunk at the most: the lane quarter's whole strip
    while (t > 0 && 4 * (1 << t) * (int64_t)k > kWideCap) --t;
    r.tshift = t; r.gper = 16 >> t; r.rows = 4 << t; r.per_chunk = 4 * r.gper;
  } else {
    r.gper = 1; r.rows = 8; r.per_chunk = 32;
  }
  return r;
}

struct AllowPlan {
  int rc;
  RankPlan base;     // the masked k <= 64 plan of the same call (nu = 1, 256-row chunks); excl: the call has sets
  AllowRule rule;
  int groups;
  int n_launches;
  RankLaunch launch[8];
};

static AllowPlan allow_plan(const srfrd_layout& lay, int B, int k, int64_t item_lo, int64_t item_hi, bool excl, int switches, int n_cu) {
  AllowPlan p = {};
  p.base = rank_plan(lay, SRFRD_RANK_TOPK, B, k < 64 ? k : 64, item_lo, item_hi, true, switches, n_cu);
  if (p.base.rc) { p.rc = p.base.rc; return p; }
  p.base.excl = excl;
  const RankPlan& r = p.base;
  if (r.stream16 && (r.nu != 1 || r.crows != 256)) { p.rc = SRFRD_E_UNSUPPORTED; return p; }      // (what the masked plan yields)
  p.rule = allow_rule(r.stream16, k, item_hi - item_lo);
  p.groups = p.rule.path == kWideAll ? 0 : r.stream_chunks * p.rule.per_chunk;
  const RankLaunch* pa = wide_find(r, kTopkMax16, kTopkMax);        // the masked stream pass: grid, block, LDS with the EXCL part
  const auto add = [&](int kernel, int64_t g, int block, int64_t lds) { p.launch[p.n_launches++] = {kernel, (int)g, block, lds}; };
  if (excl) add(kExclPrep, B, 1024, 0);
  if (p.rule.path == kWideFine) add(r.stream16 ? kAllowMax16 : kAllowMaxF32, pa->grid, pa->block, pa->lds);
  add(kWideTau, B, 256, 0);
  add(r.stream16 ? kAllowCollect16 : kAllowCollect, pa->grid, pa->block, pa->lds);
  add(kWideSelect, B, kWideBlock, (int64_t)kWideCap * 8);
  add(kAllowFallback, B, kWideBlock, 0);
  return p;
}

static void allow_launch_name(const RankPlan& r, const RankLaunch& l, char* buf, int len) {
  const char *se = r.split_e ? "true" : "false", *x = r.excl ? "true" : "false";
  switch (l.kernel) {
    case kAllowMax16: snprintf(buf, len, "srfrd::allow_max16_kernel<%s,%s>", se, x); return;
    case kAllowMaxF32: snprintf(buf, len, "srfrd::allow_max_kernel<%s>", x); return;
    case kAllowCollect16: snprintf(buf, len, "srfrd::allow_collect16_kernel<%s,%s>", se, x); return;
    case kAllowCollect: snprintf(buf, len, "srfrd::allow_collect_kernel<%s>", x); return;
    case kAllowFallback: snprintf(buf, len, "srfrd::allow_fallback_kernel"); return;
    case kAllowCount16: snprintf(buf, len, "srfrd::allow_count16_kernel<%s,%s>", se, x); return;
    case kAllowCount: snprintf(buf, len, "srfrd::allow_count_kernel<%s>", x); return;
    case kWideTau: snprintf(buf, len, "srfrd::wide_tau_kernel"); return;
    case kWideSelect: snprintf(buf, len, "srfrd::wide_select_kernel"); return;
    default: launch_name(r, l, buf, len);
  }
}

// workspace: [group maxima B * 32 ceil(n_rows / 256) f32][tau B f32][cursor B + 4 i32][candidates B * kWideCap][(chunk, lane
// quarter) maxima B * 4 ceil(n_rows / 256) f32].  32 per chunk is the fp32 stream's count and covers stream16's 16 at the most.
static int64_t allow_off(int B, int64_t n_rows, int which) {
  const int64_t nc = (n_rows + 255) / 256;
  const int64_t sizes[5] = {(int64_t)B * 32 * nc * 4, (int64_t)B * 4, ((int64_t)B + 4) * 4, (int64_t)B * kWideCap * (int64_t)sizeof(Cand),
                            (int64_t)B * nc * 16};
  int64_t off = 0;
  for (int i = 0; i < which; ++i) off += (sizes[i] + 255) & ~255ll;
  return off;
}

static int allow_args_check(const srfrd_layout* lay, const uint32_t* allow_words, int n_groups, int64_t words_per_group) {
  if (!allow_words || n_groups < 1 || words_per_group < srfrd_item_mask_words((int64_t)lay->n_items + 1)) return SRFRD_E_ARG;
  return 0;
}

}  // namespace srfrd

extern "C" int64_t srfrd_item_mask_words(int64_t n_rows) { return n_rows <= 0 ? 0 : (n_rows + 31) / 32 + 1; }

extern "C" int srfrd_item_mask_pack(const uint8_t* mask, int n_groups, int64_t n_rows, uint32_t* words, void* stream) {
  if (!mask || !words || n_groups < 1 || n_rows < 1) return SRFRD_E_ARG;
  if (n_rows >= (int64_t)INT32_MAX - 1024) return SRFRD_E_UNSUPPORTED;
  const int64_t W = srfrd_item_mask_words(n_rows);
  const dim3 grid((unsigned)((W * 32 + 255) / 256), (unsigned)(n_groups < 1024 ? n_groups : 1024));
  hipLaunchKernelGGL(item_mask_pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, mask, n_groups, n_rows, W, words);
  return (int)hipGetLastError();
}

extern "C" int srfrd_topk_allow_plan(const srfrd_layout* lay, int B, int k, int64_t item_lo, int64_t item_hi, int excl, int switches,
                                     int n_cu, int max_launches, char* names, int name_len, int32_t* geom, int32_t* sizes) {
  if (!lay || B <= 0 || k < 1 || k > kWideMax || item_lo < 0 || item_hi <= item_lo || item_hi > (int64_t)lay->n_items + 1 ||
      n_cu <= 0 || max_launches < 0)
    return SRFRD_E_ARG;
  const AllowPlan p = allow_plan(*lay, B, k, item_lo, item_hi, excl != 0, switches, n_cu);
  if (p.rc) return p.rc;
  for (int i = 0; i < p.n_launches && i < max_launches; ++i) {
    const RankLaunch& l = p.launch[i];
    if (names && name_len > 0) allow_launch_name(p.base, l, names + (int64_t)i * name_len, name_len);
    if (geom) { geom[3 * i] = l.grid; geom[3 * i + 1] = l.block; geom[3 * i + 2] = (int32_t)l.lds; }
  }
  if (sizes) { sizes[0] = p.rule.path; sizes[1] = kWideCap; sizes[2] = p.groups; }
  return p.n_launches;
}

extern "C" int64_t srfrd_topk_allow_workspace_bytes(int B, int k, int64_t n_rows) {
  if (B <= 0 || k < 1 || k > kWideMax || n_rows <= 0) return 0;
  return allow_off(B, n_rows, 5);
}

extern "C" int srfrd_logits_topk_allow(const srfrd_layout* lay, const void* item_table, const float* dense, const float* hidden,
                                       int B, int L, int64_t item_lo, int64_t item_hi, int exclude_pad, const int64_t* user_label,
                                       int k, const int64_t* excl_ptr, const int32_t* excl_items, int max_row, int64_t* topk_idx,
                                       float* topk_val, void* workspace, int64_t ws_bytes, void* excl_workspace,
                                       const uint32_t* allow_words, int n_groups, int64_t words_per_group,
                                       const int64_t* allow_group, void* stream) {
  if (!topk_idx || !topk_val || !workspace || k < 1 || k > kWideMax) return SRFRD_E_ARG;
  if (int rc = topk_args_check(lay, item_table, dense, hidden, B, L, item_lo, item_hi, user_label)) return rc;
  if (ws_bytes < srfrd_topk_allow_workspace_bytes(B, k, item_hi - item_lo)) return SRFRD_E_ARG;
  if (int rc = allow_args_check(lay, allow_words, n_groups, words_per_group)) return rc;
  if (int rc = excl_args(excl_ptr, excl_items, max_row, excl_workspace, B, item_hi)) return rc;
  const AllowPlan p = allow_plan(*lay, B, k, item_lo, item_hi, excl_ptr != nullptr, read_switches(), num_cu());
  if (p.rc) return p.rc;
  const int64_t n_rows = item_hi - item_lo;
  // the maxima of every plan fit the query's 32 per 256 rows; held here because a plan past it would write past them
  if (p.groups > 32 * ((n_rows + 255) / 256)) return SRFRD_E_DEVICE;
  const RankPlan& r = p.base;
  RankIO io = {excl_ptr, excl_items, max_row, topk_idx, topk_val};
  TopkArgs a = rank_args(r, lay, item_table, dense, hidden, B, L, item_lo, item_hi, exclude_pad, user_label, k, max_row,
                         excl_workspace, io);
  char* ws = (char*)workspace;
  WideArgs w = {};
  w.gmax = a.cmax = (float*)(ws + allow_off(B, n_rows, 0));
  a.tau = (float*)(ws + allow_off(B, n_rows, 1));
  a.ccnt = (int32_t*)(ws + allow_off(B, n_rows, 2));
  a.cand = (Cand*)(ws + allow_off(B, n_rows, 3));
  w.gstride = p.rule.path == kWideAll ? 1 : p.groups;
  w.cmx = w.gmax; w.cstride = w.gstride; w.cmul = 1;
  if (p.rule.path == kWideFine && r.stream16) { w.cmx = (float*)(ws + allow_off(B, n_rows, 4)); w.cstride = r.stream_chunks * 4; w.cmul = 4; }
  w.gper = p.rule.gper; w.tshift = p.rule.tshift; w.cap = kWideCap; w.excl = excl_ptr != nullptr;
  const AllowArgs f = {allow_words, allow_group, n_groups, (int)(srfrd_item_mask_words((int64_t)lay->n_items + 1) - 2), words_per_group};
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < p.n_launches; ++i) {
    const RankLaunch& l = p.launch[i];
    int rc = 0;
    switch (l.kernel) {
      case kAllowMax16:
        rc = with_flag(r.excl, [&](auto x) { return with_flag(r.split_e, [&](auto se) {
          return launch_rank(allow_max16_kernel<decltype(se)::value, decltype(x)::value>, l, st, a, w, f); }); });
        break;
      case kAllowMaxF32: rc = with_flag(r.excl, [&](auto x) { return launch_rank(allow_max_kernel<decltype(x)::value>, l, st, a, w, f); }); break;
      case kWideTau: rc = launch_rank(wide_tau_kernel, l, st, a, w); break;
      case kAllowCollect16:
        rc = with_flag(r.excl, [&](auto x) { return with_flag(r.split_e, [&](auto se) {
          return launch_rank(allow_collect16_kernel<decltype(se)::value, decltype(x)::value>, l, st, a, w, f); }); });
        break;
      case kAllowCollect: rc = with_flag(r.excl, [&](auto x) { return launch_rank(allow_collect_kernel<decltype(x)::value>, l, st, a, w, f); }); break;
      case kWideSelect: rc = launch_rank(wide_select_kernel, l, st, a, w, topk_idx, topk_val); break;
      case kAllowFallback: rc = launch_rank(allow_fallback_kernel, l, st, a, w, f, topk_idx, topk_val); break;
      default: rc = launch_one(r, l, a, io, st);        // the exclusion pre-pass
    }
    if (rc) return rc;
  }
  return 0;
}

extern "C" int srfrd_target_rank_allow(const srfrd_layout* lay, const void* item_table, const float* dense, const float* hidden,
                                       int B, int L, int64_t item_lo, int64_t item_hi, int exclude_pad, const int64_t* user_label,
                                       const int64_t* targets, const int64_t* excl_ptr, const int32_t* excl_items, int max_row,
                                       int cut_k, int32_t* rank, double* metric_acc, void* workspace,
                                       const uint32_t* allow_words, int n_groups, int64_t words_per_group,
                                       const int64_t* allow_group, void* stream) {
  if (!targets || !rank || !workspace || cut_k <= 0) return SRFRD_E_ARG;
  if (int rc = topk_args_check(lay, item_table, dense, hidden, B, L, item_lo, item_hi, user_label)) return rc;
  if (int rc = allow_args_check(lay, allow_words, n_groups, words_per_group)) return rc;
  if (int rc = excl_args(excl_ptr, excl_items, max_row, workspace, B, item_hi)) return rc;
  // the masked plan's geometry (one user tile per wave, 256-row chunks), whether or not the call carries sets
  RankPlan p = rank_plan(*lay, metric_acc ? SRFRD_RANK_TARGET_METRIC : SRFRD_RANK_TARGET, B, 1, item_lo, item_hi, true,
                         read_switches(), num_cu());
  if (p.rc) return p.rc;
  p.excl = excl_ptr != nullptr;
  RankIO io = {excl_ptr, excl_items, max_row, nullptr, nullptr, targets, cut_k, metric_acc};
  TopkArgs a = rank_args(p, lay, item_table, dense, hidden, B, L, item_lo, item_hi, exclude_pad, user_label, 1, max_row, workspace, io);
  a.tau = (float*)workspace;                     // s_t
  a.ccnt = rank;
  const AllowArgs f = {allow_words, allow_group, n_groups, (int)(srfrd_item_mask_words((int64_t)lay->n_items + 1) - 2), words_per_group};
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < p.n_launches; ++i) {
    const RankLaunch& l = p.launch[i];
    int rc = 0;
    switch (l.kernel) {
      case kExclPrep: rc = p.excl ? launch_one(p, l, a, io, st) : 0; break;
      case kTargetCount16:
        rc = with_flag(p.excl, [&](auto x) { return with_flag(p.split_e, [&](auto se) {
          return launch_rank(allow_count16_kernel<decltype(se)::value, decltype(x)::value>, l, st, a, f); }); });
        break;
      case kTargetCount: rc = with_flag(p.excl, [&](auto x) { return launch_rank(allow_count_kernel<decltype(x)::value>, l, st, a, f); }); break;
      default: rc = launch_one(p, l, a, io, st);      // the target's score (unchanged) and the metric
    }
    if (rc) return rc;
  }
  return 0;
}
