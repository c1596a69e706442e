// The device key sort (include/srfrd_hip_sort.h): a stable least-significant-digit radix sort of int64 item
// ids through a 32-bit transformed key with a 32-bit index as payload.  Included by srfrd_optim.hip (after srfrd_dev.h: the
// workgroup barriers below are that header's __syncthreads, which the SRFRD_SKEW builds follow with a sleep of half the waves).
//
// A pass over one digit (<= 8 bits) is three launches, and the only dependency between workgroups is the launch boundary:
//   count    tile t -> hist[d][t] = how many of its elements hold digit d              (every entry written: nothing is zeroed)
//   rows     row d  -> hist[d][t] = sum of hist[d][t' < t]  (in place),  dtot[d] = the row's total
//   scatter  tile t -> element e to  base[d] + hist[d][t] + (its rank among the tile's elements of digit d),
//                      base[d] = sum of dtot[d' < d], scanned again by every workgroup (256 words)
// A tile is 256 threads x 8 elements; wave w owns the 512 consecutive positions behind tile_base + 512 w, element i of lane l at
// + 64 i + l: position order is (wave, i, lane).  The rank of an element among the equal digits of its tile follows that order and
// nothing else: within a wave instruction from __ballot matches (the lanes below mine that hold my digit), across instructions
// from a per-wave counter only the match's lowest lane writes, across waves from a scan of the per-wave counters in wave order.
// No atomic anywhere: an atomic's arrival order is not the position order.
#pragma once

namespace srfrd {

constexpr int kSortItems = 8;                  // elements per thread
constexpr int kSortWaves = 4;                  // waves per workgroup (256 threads)
constexpr int kSortTile = 256 * kSortItems;    // elements per workgroup
constexpr int kSortRadix = 256;                // rows of hist: a digit has at most 8 bits; a narrower digit leaves the upper rows zero

// The sort key: invalid ids go to the two ends of the list (below the pad key 0 and above key_max), where the table reductions
// skip them; nothing is ever indexed by it.
__device__ __forceinline__ uint32_t sort_u(int64_t key, int64_t key_max) {
  return key < 0 ? 0u : (key > key_max ? (uint32_t)(key_max + 2) : (uint32_t)(key + 1));
}

// position of element i of this thread
__device__ __forceinline__ uint32_t sort_pos(int i) {
  return blockIdx.x * (uint32_t)kSortTile + (threadIdx.x >> 6) * (uint32_t)(64 * kSortItems) + (uint32_t)(64 * i) + (threadIdx.x & 63);
}

// exclusive scan of one value per thread over the 256 threads, in thread order; `total`: the sum.  wtot: kSortWaves words of LDS
__device__ __forceinline__ uint32_t sort_block_scan(uint32_t v, uint32_t* wtot, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();                               // (the last use of wtot is over)
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kSortWaves; ++w) {
    const uint32_t t = wtot[w];
    before += w < wave ? t : 0u;
    total += t;
  }
  return before + incl - v;
}

// Ranks of the tile's elements among equal digits.  digit[i] / valid: this thread's elements (bit i of `valid`: inside the
// list).  cnt: [kSortWaves][kSortRadix] words of LDS.  On return (behind a barrier) rank[i] counts the elements of the same
// digit ahead of element i IN ITS WAVE and cnt[w][d] is wave w's count of digit d.
__device__ __forceinline__ void sort_tile_ranks(const uint32_t (&digit)[kSortItems], uint32_t valid, int bits, uint32_t* cnt,
                                                uint32_t (&rank)[kSortItems]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = threadIdx.x; d < kSortWaves * kSortRadix; d += 256) cnt[d] = 0;
  __syncthreads();
  volatile uint32_t* wc = cnt + wave * kSortRadix;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const bool ok = (valid >> i) & 1u;
    unsigned long long match = __ballot(ok);     // -> the lanes of this wave whose element i is in the list and holds my digit
    for (int b = 0; b < bits; ++b) {
      const bool one = (digit[i] >> b) & 1u;
      const unsigned long long vote = __ballot(one);
      match &= one ? vote : ~vote;
    }
    const unsigned long long ahead = match & below;
    uint32_t seen = 0;
    if (ok) seen = wc[digit[i]];                 // what the earlier instructions of this wave counted: every lane of the match reads it ...
    rank[i] = seen + (uint32_t)__popcll(ahead);
    __builtin_amdgcn_wave_barrier();
    if (ok && ahead == 0) wc[digit[i]] = seen + (uint32_t)__popcll(match);      // ... before its lowest lane moves it on
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
}

// this thread's elements of pass input: the int64 keys with the position as index (FIRST), else the last pass's pair
template <bool FIRST>
__device__ __forceinline__ uint32_t sort_load(const int64_t* __restrict__ keys, int64_t key_max, const uint32_t* __restrict__ in_key,
                                              const uint32_t* __restrict__ in_idx, uint32_t n, uint32_t (&k)[kSortItems],
                                              uint32_t (&idx)[kSortItems]) {
  uint32_t valid = 0;
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const uint32_t pos = sort_pos(i);
    k[i] = 0;
    idx[i] = 0;
    if (pos < n) {
      valid |= 1u << i;
      if (FIRST) {
        k[i] = sort_u(keys[pos], key_max);
        idx[i] = pos;
      } else {
        k[i] = in_key[pos];
        idx[i] = in_idx[pos];
      }
    }
  }
  return valid;
}

template <bool FIRST>
__global__ void __launch_bounds__(256) keysort_count_kernel(const int64_t* __restrict__ keys, int64_t key_max,
                                                           const uint32_t* __restrict__ in_key, uint32_t n, int shift, int bits,
                                                           uint32_t* __restrict__ hist, uint32_t n_tiles) {
  __shared__ uint32_t cnt[kSortWaves * kSortRadix];
  uint32_t k[kSortItems], idx[kSortItems], digit[kSortItems], rank[kSortItems];
  const uint32_t valid = sort_load<FIRST>(keys, key_max, in_key, in_key, n, k, idx);
  const uint32_t mask = (1u << bits) - 1u;
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) digit[i] = (k[i] >> shift) & mask;
  sort_tile_ranks(digit, valid, bits, cnt, rank);
  uint32_t total = 0;                            // thread d: the tile's count of digit d
#pragma unroll
  for (int w = 0; w < kSortWaves; ++w) total += cnt[w * kSortRadix + threadIdx.x];
  hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = total;
}

// workgroup d: row d of hist to its exclusive prefix over the tiles, 256 at a time with a carry
__global__ void __launch_bounds__(256) keysort_rows_kernel(uint32_t* __restrict__ hist, uint32_t n_tiles, uint32_t* __restrict__ dtot) {
  __shared__ uint32_t wtot[kSortWaves];
  uint32_t* row = hist + (size_t)blockIdx.x * n_tiles;
  uint32_t carry = 0;
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t v = t < n_tiles ? row[t] : 0u;
    uint32_t total;
    const uint32_t ex = sort_block_scan(v, wtot, total);
    if (t < n_tiles) row[t] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) dtot[blockIdx.x] = carry;
}

// LAST: the pass that writes the result - order[j] as int64 and sorted_keys[j] = keys[order[j]], the original 64-bit value
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) keysort_scatter_kernel(const int64_t* __restrict__ keys, int64_t key_max,
                                                             const uint32_t* __restrict__ in_key, const uint32_t* __restrict__ in_idx,
                                                             uint32_t n, int shift, int bits, const uint32_t* __restrict__ hist,
                                                             const uint32_t* __restrict__ dtot, uint32_t n_tiles,
                                                             uint32_t* __restrict__ out_key, uint32_t* __restrict__ out_idx,
                                                             int64_t* __restrict__ sorted_keys, int64_t* __restrict__ order) {
  __shared__ uint32_t cnt[kSortWaves * kSortRadix];
  __shared__ uint32_t wtot[kSortWaves];
  uint32_t k[kSortItems], idx[kSortItems], digit[kSortItems], rank[kSortItems];
  const uint32_t valid = sort_load<FIRST>(keys, key_max, in_key, in_idx, n, k, idx);
  const uint32_t mask = (1u << bits) - 1u;
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) digit[i] = (k[i] >> shift) & mask;
  // thread d: where this tile's elements of digit d begin in the output
  uint32_t total;
  uint32_t first = sort_block_scan(dtot[threadIdx.x], wtot, total) + hist[(size_t)threadIdx.x * n_tiles + blockIdx.x];
  sort_tile_ranks(digit, valid, bits, cnt, rank);
#pragma unroll
  for (int w = 0; w < kSortWaves; ++w) {         // the per-wave counts, in wave order -> where wave w's elements of digit d begin
    const uint32_t c = cnt[w * kSortRadix + threadIdx.x];
    cnt[w * kSortRadix + threadIdx.x] = first;
    first += c;
  }
  __syncthreads();
  const uint32_t* wc = cnt + (threadIdx.x >> 6) * kSortRadix;
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    if (!((valid >> i) & 1u)) continue;
    const uint32_t to = wc[digit[i]] + rank[i];
    if (to >= n || idx[i] >= n) continue;        // (cannot happen: the counts add up to n.  A wrong count must not become a stray store)
    if (LAST) {
      order[to] = (int64_t)idx[i];
      // a valid id is its sort key less one; only an invalid id's 64-bit value has to be fetched from where it came
      sorted_keys[to] = (k[i] >= 1u && (int64_t)k[i] <= key_max + 1) ? (int64_t)k[i] - 1 : keys[idx[i]];
    } else {
      out_key[to] = k[i];
      out_idx[to] = idx[i];
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// The workspace: [dtot: 256 words | hist: 256 x n_tiles words | two (key, index) pairs of n words each, every array on a
// 16-byte boundary].  Its size depends on n alone, so it never shrinks when key_max grows.
struct KeySortPlan {
  int passes, digit_bits;
  uint32_t n_tiles;
  int64_t off_hist, off_pair[2][2], bytes;
};

inline bool keysort_plan(int64_t n, int64_t key_max, KeySortPlan* p) {
  if (n < 0 || n > 2147483647ll || key_max < 0 || key_max > 2147483645ll) return false;
  int bits = 0;
  for (int64_t v = key_max + 2; v > 0; v >>= 1) ++bits;      // bit length of the largest sort key
  p->passes = (bits + 7) / 8;
  p->digit_bits = (bits + p->passes - 1) / p->passes;
  const int64_t tiles = (n + kSortTile - 1) / kSortTile;
  p->n_tiles = (uint32_t)(tiles > 0 ? tiles : 1);
  const int64_t words = (n * 4 + 15) / 16 * 16;
  int64_t off = kSortRadix * 4;
  p->off_hist = off;
  off += (int64_t)kSortRadix * p->n_tiles * 4;
  for (int b = 0; b < 2; ++b)
    for (int a = 0; a < 2; ++a) {
      p->off_pair[b][a] = off;
      off += words;
    }
  p->bytes = off;
  return true;
}

}  // namespace srfrd
