// Shared pieces of the fused encoder translation units (forward / backward): launch arguments, the LayerNorm
// parameter cache, debug taps, the launchers' helpers.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "srfrd_dev.h"
#include "srfrd_enc_plan.h"

namespace SRFRD_NS {

struct EncArgs {
  Dims dm;
  const float* table;       // fp32 item table, or NULL when the gathers read the bf16 shadow
  const uint16_t* table16;  // bf16 shadow of the item table (srfrd_layout::table_bf16), or NULL
  const float* dense;
  const float* packed;      // srfrd_pack_weights output (MFMA-fragment-ordered weights)
  const int64_t *in_ids, *fk_ids, *pos_ids, *pos_fk, *neg_ids, *neg_fk;
  int B, L;
  uint32_t seed;
  const uint32_t* seed_dev;
  uint32_t drop_thr;
  float drop_scale;
  int drop_on;
  int64_t seq0;
  float qscale;
  // forward outputs
  float *hidden, *pos_logits, *neg_logits, *save_x, *save_h1, *save_aux, *loss_part;
  // backward inputs / outputs
  const float *c_hidden, *c_pl, *c_nl, *c_save_x, *c_save_h1, *c_save_aux, *d_hidden, *d_pos, *d_neg;
  int fused_bce;
  int last_only;       // forward, inference: only the LAST position's hidden state is wanted (hidden is (B, d_out))
  float *grad_table, *grad_slabs;
  float* contrib;      // deterministic table scatter: (3, B, L, d_item) row contributions instead of float atomics (or NULL)
  // SRFRD_BUF_GLOBAL build only: per-workgroup working-set scratch (floats) in global memory
  float* scratch;
  int64_t scratch_stride;
  int lds_floats;      // dynamic LDS (floats) the long build may carve from before falling back to `scratch`
  // debug taps
  float* dbg;
  int dbg_seq;
  int64_t dbg_slot;
  // ragged kernels (seq_len 50): sequence -> workgroup schedule from srfrd_seq_order's per-sequence lengths (NULL: b = blockIdx.x, += gridDim.x)
  const int* sched;    // int32 workspace, layout below (kSched*)
  int sched_mode;      // 0 none, 1 length order (workgroup x takes the sequence of rank perm(x): see rag_take)
  int ragged_off;      // diagnostic: the ragged kernels compute every row (t0 = 0), as the full kernels do
  // ragged train kernel, srfrd_encoder_train_ranked: > 0 = length order with this pair stride and NO workspace - every workgroup
  // finds the batch's first-item positions itself (rag_rank_batch); 0: `sched` decides.  (The two words stand where a pointer
  // no kernel read any more stood: the argument block keeps its size, every kernel its implicit-argument offsets.)
  int rank_G;
  int rank_pad_;
};

// Schedule workspace (int32), filled by srfrd_seq_order for ONE batch:
//   [kSchedG]        pair stride G (workgroups of the "first round": the CU count)
//   [kSchedT0 + b]   first non-pad position t0 of sequence b (L: all padding)
// The ragged kernels rank the sequences themselves (longest first = smallest t0 first, ties by index - a function of the
// batch, so the summation order of the dense-gradient slabs is too): every workgroup selects the ONE sequence of the rank
// it wants from the B lengths (a 64-bucket histogram in LDS + a ballot scan: rag_select) instead of a sort kernel ahead of
// the launch - a one-workgroup sort costs more dependent memory round trips than it saves.
constexpr int kSchedG = 0, kSchedT0 = 16;
__host__ __device__ __forceinline__ int64_t sched_ints(int B) { return kSchedT0 + (int64_t)B; }

}  // namespace SRFRD_NS

#include "srfrd_enc_bwd_head.h"      // kHeadRows: the per-position arrays that the LDS sizes below count

namespace SRFRD_NS {

// Checkpoint layout: SEQUENCE-major.  Everything the backward reads back for sequence b is contiguous per buffer -
// save_x: (nb + 1) blocks of [L][D] at b * (nb + 1) * L * D; save_h1: nb blocks at b * nb * L * D; save_aux
// (srfrd_aux_floats): nb blocks of aux_seq_floats at b * nb * aux_seq_floats, each the planes r, o, q, k, v [L][D] and
// Pm [H][L][LP] (one probability block per attention head).  (A block-major layout put the ten planes a workgroup touches per block 10 MB apart at BASELINE
// configs[3]: every first access of a phase was a TLB miss on the sequence's critical path.)
__host__ __device__ __forceinline__ int64_t aux_seq_floats(int L, int LP, int D, int H = 1) { return 5ll * L * D + (int64_t)H * L * LP; }
__host__ __device__ __forceinline__ int64_t x_off(int i, int b, int nb, int L, int D) { return ((int64_t)b * (nb + 1) + i) * L * D; }
__host__ __device__ __forceinline__ int64_t h1_off(int i, int b, int nb, int L, int D) { return ((int64_t)b * nb + i) * L * D; }
struct AuxOff {
  int64_t r, o, q, k, v, p;
};
__host__ __device__ __forceinline__ AuxOff aux_off(int i, int b, int nb, int L, int LP, int D, int H = 1) {
  const int64_t blk = ((int64_t)b * nb + i) * aux_seq_floats(L, LP, D, H), plane = (int64_t)L * D;
  AuxOff f;
  f.r = blk;
  f.o = blk + plane;
  f.q = blk + 2 * plane;
  f.k = blk + 3 * plane;
  f.v = blk + 4 * plane;
  f.p = blk + 5 * plane;
  return f;
}

// Scope and sizing of the long-sequence and seq_len-50 kernels (read by the kernels and by the kernel plan below).
// Row-owner forward (srfrd_encoder_fwd_rows_kernel.inc): hidden width 50, 8 waves, seq_len <= 16 * kRowMaxTiles.
constexpr int kRowWaves = 8;
constexpr int kRowMaxTiles = 13;         // S^T accumulators a lane holds: key tiles of a query tile (seq_len <= 208)
__host__ __device__ constexpr int64_t rows_lds_floats(int L, int D, int n_blocks) {
  const int LP = (L + 15) & ~15, DS = ((D + 3) & ~3) + 2;
  return 2ll * LP * DS + (int64_t)kRowWaves * 2 * 16 * DS + 5ll * LP + 64 + ln_cache_floats(n_blocks) + kSlack;
}
// Slot-placed backward (srfrd_encoder_bwd_slots_kernel.inc): seq_len 50 and 100.
constexpr int kSlotWaves = 8;
__host__ __device__ constexpr int slots_R(int L) { return (L + 3) & ~3; }
__host__ __device__ constexpr int64_t slots_lds_floats(int L, int D, int n_blocks) {
  const int LP = (L + 15) & ~15, DS = ((D + 3) & ~3) + 2;
  // six slots; the head's per-position arrays, s_delta and a spare one; s_misc
  return 6ll * slots_R(L) * DS + (kHeadRows + 2ll) * LP + 64 + 2ll * ln_cache_floats(n_blocks) + kSlack;
}
// Row-chunked backward (srfrd_encoder_bwd_chunks_kernel.inc): seq_len 17..208, three [L][D] intermediates in scratch.
constexpr int kCkWaves = 8;
constexpr int kCkRows = 48;            // rows of a chunk (three 16-row tiles)
__host__ __device__ constexpr int64_t chunks_lds_floats(int L, int D, int n_blocks) {
  const int LP = (L + 15) & ~15, DS = ((D + 3) & ~3) + 2, LR = (L + 3) & ~3;
  // K | V, then a pool that is the score chunk + two chunk slots (attention pass) or five chunk slots (projection pass)
  const int64_t pool_att = (int64_t)kCkRows * (LR + 2) + 2ll * kCkRows * DS, pool_prj = 5ll * kCkRows * DS;
  return 2ll * LR * DS + (pool_att > pool_prj ? pool_att : pool_prj) + (kHeadRows + 2ll) * LP + 64 + 2ll * ln_cache_floats(n_blocks) + kSlack;
}
__host__ __device__ constexpr int64_t chunks_scratch_floats(int L, int D) { return 3ll * (((L + 3) & ~3) * D + 64); }
// Ragged backward (srfrd_encoder_bwd_ragged_kernel.inc): seq_len 50, hidden 50.
// Per-sequence working sets (floats) of the ragged pair, without the LayerNorm caches:
constexpr int kRagFwdWork = 64 * 66 + 4 * 64 * 54 + 4 * 64 + 64;    // scores / x [64][66], four [64][54], 4 per-row arrays, misc
// guard (12 rows), six [52][54] slots, the head's per-row arrays + s_delta, s_brep, s_dummy, misc
constexpr int kRagBwdWork = 12 * 54 + 6 * 52 * 54 + (kHeadRows + 3) * 64 + 64;
__host__ __device__ constexpr int64_t bwd_ragged_lds_floats(int n_blocks) {
  // working set + two LayerNorm caches + slack
  return kRagBwdWork + 2ll * ln_cache_floats(n_blocks) + kSlack;
}
// Ragged train kernel (srfrd_encoder_train_ragged.hip): the forward's and the backward's working sets overlay each other,
// then the LayerNorm parameters and the backward's gradient accumulators.  The forward's tile over-reads behind its last
// matrix land in its own per-row arrays: no slack.  Never larger than bwd_ragged_lds_floats (two workgroups per CU).
__host__ __device__ constexpr int64_t train_ragged_lds_floats(int n_blocks) {
  return (kRagFwdWork > kRagBwdWork ? kRagFwdWork : kRagBwdWork) + 2ll * ln_cache_floats(n_blocks);
}
static_assert(kRagFwdWork <= kRagBwdWork + kSlack, "train kernel LDS within the backward's");

// Optimisation barrier on a wave-uniform pointer: stops LLVM from hoisting the per-call-site address arithmetic of
// ~35 inlined GEMMs out of the sequence / block loops (which costs > 256 VGPRs and spills).
__device__ __forceinline__ void launder(lds_f*& p) {
  asm volatile("" : "+s"(p));
}
#ifndef SRFRD_BUF_GLOBAL
__device__ __forceinline__ void launder(const float*& p) {
  asm volatile("" : "+s"(p));
}
__device__ __forceinline__ void launder(float*& p) {
  asm volatile("" : "+s"(p));
}
#endif

// Diagnostic build only (tools/phase_profile.py compiles a copy with -DSRFRD_STAMPS and a STAMP(n) after every
// workgroup barrier): thread 0 adds the s_memtime delta of each phase into a per-workgroup table that aliases the
// debug-tap buffer.  The shipped library contains no stamp.
#ifdef SRFRD_STAMPS
// (accumulated in LDS and flushed once: a global read-modify-write per stamp would put a memory round trip of its own
// into every phase it measures)
#define STAMP_INIT __shared__ unsigned long long stamp_lds[128]; \
                   if (threadIdx.x < 128) stamp_lds[threadIdx.x] = 0; \
                   __syncthreads(); \
                   unsigned long long stamp_prev = __builtin_amdgcn_s_memtime();
#define STAMP(id) do { if (threadIdx.x == 0) { unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
                       stamp_lds[id] += t_ - stamp_prev; stamp_prev = t_; } } while (0)
#define STAMP_FLUSH do { __syncthreads(); if (threadIdx.x < 128 && a.dbg) \
                       ((unsigned long long*)a.dbg)[(int64_t)blockIdx.x * 128 + threadIdx.x] = stamp_lds[threadIdx.x]; } while (0)
#else
#define STAMP_INIT
#define STAMP(id) do {} while (0)
#define STAMP_FLUSH do {} while (0)
#endif

// A contiguous [rows][cols] fp32 block of global memory on its way into an LDS matrix [rows][ld].  load() puts every
// element the thread owns in flight at once: indices past the end are clamped instead of predicated, so the loads are
// unconditional, stay back to back, and the block costs ONE memory round trip (a `for (i = tid; ...) lds[..] = g[i]`
// loop that the compiler does not unroll pays one round trip - 1.5 to 2 k cycles from L2 / HBM here - per iteration).
// store() writes them to LDS; a caller may put independent work between the two.  V2: 8-byte accesses (cols even and
// the block 8-byte aligned).  One G2L covers ITER * blockDim elements (pairs); copy_g2l walks larger blocks in chunks.
typedef float f32x2 __attribute__((ext_vector_type(2)));
#ifdef SRFRD_BUF_GLOBAL
typedef f32x2 lds_f2;
#else
typedef __attribute__((address_space(3))) f32x2 lds_f2;
#endif
template <int ITER, bool V2>
struct G2L {
  float v[ITER][V2 ? 2 : 1];
  __device__ __forceinline__ void load(const float* src, int rows, int cols, int nthr, int base = 0) {
    const int n = V2 ? rows * (cols >> 1) : rows * cols;
#pragma unroll
    for (int u = 0; u < ITER; ++u) {
      const int i = min(base + u * nthr + (int)threadIdx.x, n - 1);
      if constexpr (V2) {
        const f32x2 t = reinterpret_cast<const f32x2*>(src)[(unsigned)i];
        v[u][0] = t.x; v[u][1] = t.y;
      } else {
        v[u][0] = src[(unsigned)i];
      }
    }
  }
  // [rows][cols] window of a row-major global matrix whose rows are `sld` floats apart (V2: cols, sld even)
  __device__ __forceinline__ void load2d(const float* src, int rows, int cols, int sld, int nthr) {
    const int cw = V2 ? cols >> 1 : cols, n = rows * cw;
#pragma unroll
    for (int u = 0; u < ITER; ++u) {
      const int i = min(u * nthr + (int)threadIdx.x, n - 1);
      const int t = i / cw, c = i - t * cw;
      if constexpr (V2) {
        const f32x2 w = *reinterpret_cast<const f32x2*>(src + (unsigned)(t * sld + 2 * c));
        v[u][0] = w.x; v[u][1] = w.y;
      } else {
        v[u][0] = src[(unsigned)(t * sld + c)];
      }
    }
  }
  __device__ __forceinline__ void store(lds_f* dst, int ld, int rows, int cols, int nthr, int base = 0) const {
    const int cw = V2 ? cols >> 1 : cols, n = rows * cw;
#pragma unroll
    for (int u = 0; u < ITER; ++u) {
      const int i = base + u * nthr + (int)threadIdx.x;
      if (i < n) {
        const int t = i / cw, c = i - t * cw;
        if constexpr (V2) *reinterpret_cast<lds_f2*>(dst + t * ld + 2 * c) = f32x2{v[u][0], v[u][1]};
        else dst[t * ld + c] = v[u][0];
      }
    }
  }
};
template <int ITER, bool V2>
__device__ __forceinline__ void copy_g2l(lds_f* dst, int ld, const float* src, int rows, int cols, int nthr) {
  const int n = V2 ? rows * (cols >> 1) : rows * cols;
  for (int base = 0; base < n; base += ITER * nthr) {
    G2L<ITER, V2> g;
    g.load(src, rows, cols, nthr, base);
    g.store(dst, ld, rows, cols, nthr, base);
  }
}

// LayerNorm weights / biases -> LDS once per workgroup (read by every row pass of every sequence)
__device__ __forceinline__ void fill_ln_cache(lds_f* s_ln, const float* P, const Dims& ly) {
  const int D = ly.D;
  for (int idx = threadIdx.x; idx < (4 * ly.n_blocks + 2) * 64; idx += blockDim.x) {
    const int vec = idx >> 6, c = idx & 63;
    float v = 0.f;
    if (vec < 4 * ly.n_blocks) {
      const BlkOff o = blk_off(ly.blk0 + (vec >> 2) * ly.blk_stride, D);
      const int sel = vec & 3;
      const int off = sel == 0 ? o.ln1_w : sel == 1 ? o.ln1_b : sel == 2 ? o.ln2_w : o.ln2_b;
      if (c < D) v = P[off + c];
    } else if (c < ly.d_out) {
      v = P[(vec == 4 * ly.n_blocks ? ly.off_ll_w : ly.off_ll_b) + c];
    }
    s_ln[idx] = v;
  }
}

__device__ __forceinline__ void tap(const EncArgs& a, int b, int slot, const lds_f* buf, int rows, int cols, int ld) {
#ifdef SRFRD_STAMPS
  return;
#endif
  if (a.dbg == nullptr || b != a.dbg_seq) return;
  float* dst = a.dbg + (int64_t)slot * a.dbg_slot;
  for (int i = threadIdx.x; i < rows * cols; i += blockDim.x) {
    const int r = i / cols, c = i - r * cols;
    dst[i] = buf[r * ld + c];
  }
}

// ================================================================================================
// host side
// ================================================================================================
// kind variant -> <K, DI>: f(std::integral_constant<int, v>) for a plan's variant v (kKindVariants[v] are the arguments)
template <class F>
static int with_variant(int v, F&& f) {
  switch (v) {
    case 0: return f(std::integral_constant<int, 0>());
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    default: return f(std::integral_constant<int, 3>());
  }
}

// a plan's kind variant and flag -> template arguments: f(K, DI, flag) as integral constants, usable as <K, DI, flag>
template <class F>
static int with_variant_flag(const KernelPlan& k, F&& f) {
  return with_variant(k.variant, [&](auto v) {
    constexpr KindVariant kv = kKindVariants[decltype(v)::value];
    return with_flag(k.flag, [&](auto t) { return f(std::integral_constant<int, kv.K>(), std::integral_constant<int, kv.DI>(), t); });
  });
}

// kind variant of a layout: the hidden-50, one-head specialisations cover these kinds and width splits (-1: none)
static inline int kind_variant(const srfrd_layout& lay) {
  if (lay.D != 50 || lay.n_heads != 1) return -1;
  if (lay.kind == SRFRD_SASREC) return 0;
  if (lay.kind == SRFRD_SRFR && lay.d_item == 45) return 1;
  if (lay.kind == SRFRD_SRFRN && lay.d_item == 45) return 2;
  if (lay.kind >= SRFRD_SRFU_B && lay.d_item == 50) return 3;
  return -1;
}

// launch one instantiation as the kernel plan sized it
template <class K>
static int launch_enc(K kernel, const KernelPlan& k, void* stream, const EncArgs& a) {
  if (const int rc = lds_opt_in((const void*)kernel, k.lds)) return rc;
  hipLaunchKernelGGL(kernel, dim3(k.grid), dim3(k.threads), (size_t)k.lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

#ifndef SRFRD_BUF_GLOBAL
// one launcher per LDS-resident family, each in the translation unit that instantiates its kernels
int launch_fwd_first(const KernelPlan& k, const EncArgs& a, void* stream);    // srfrd_encoder_fwd.hip
int launch_fwd_rows(const KernelPlan& k, const EncArgs& a, void* stream);     // srfrd_encoder_fwd_rows.hip
int launch_fwd_ragged(const KernelPlan& k, const EncArgs& a, void* stream);   // srfrd_encoder_fwd_ragged.hip
int launch_bwd_first(const KernelPlan& k, const EncArgs& a, void* stream);    // srfrd_encoder_bwd.hip
int launch_bwd_ragged(const KernelPlan& k, const EncArgs& a, void* stream);   // srfrd_encoder_bwd_ragged.hip
int launch_bwd_slots(const KernelPlan& k, const EncArgs& a, void* stream);    // srfrd_encoder_bwd_slots.hip
int launch_bwd_chunks(const KernelPlan& k, const EncArgs& a, void* stream);   // srfrd_encoder_bwd_chunks.hip
int launch_train_ragged(const KernelPlan& k, const EncArgs& a, void* stream); // srfrd_encoder_train_ragged.hip
#endif

}  // namespace SRFRD_NS
