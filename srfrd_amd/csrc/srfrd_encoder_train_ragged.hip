// Ragged train kernel (seq_len 50, hidden 50): the training forward of srfrd_encoder_fwd_ragged_kernel.inc and the fused-BCE
// backward of srfrd_encoder_bwd_ragged_kernel.inc as ONE launch.  Each workgroup runs, for the sequence its schedule slot
// names, the forward, a workgroup barrier, then the backward - which reads only what the same workgroup has just written
// (checkpoints, hidden states, logits): a workgroup-scope fence is all the hand-off needs, no workgroup waits for another.
// The BCE normaliser (the global target count) enters later, in the Adam step, so nothing in here needs the whole batch.
// The forward's head also does the first part of the backward's head (SEAM_ of rag_fwd_seq / rag_bwd_seq): logit gradients,
// d hidden, the target rows' item-table contributions; the backward starts from d hidden.  What the backward's head needs
// first - the last block's output, d hidden, the ids - stays in LDS and registers across the barrier (rag_seam_handoff): its
// first arithmetic waits for no global load, and the loads it does issue stand behind no id round trip.
//
// Against the two launches: a long sequence's backward no longer waits for the slowest forward on the chip, and once its
// short partner on the CU has finished, it runs alone.  Results are those of the two launches bit for bit: same
// arithmetic, the same sequence -> workgroup schedule (so the same per-workgroup slab sums), and every phase starts from
// the zeroed working set a fresh launch starts from.
#include "srfrd_enc_common.h"

#include "srfrd_encoder_fwd_ragged_kernel.inc"
#include "srfrd_encoder_bwd_ragged_kernel.inc"

namespace srfrd {

// LDS: [ working set (forward and backward overlaid) | LayerNorm parameters | LayerNorm gradient accumulators ]
template <int K_, int DI_, bool RMW_>
__global__ void __launch_bounds__(512, 4) encoder_train_ragged_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Dims& ly = a.dm;
  constexpr int LP = 64, DS = 54, SLD = 66, nthr = 512;
  constexpr int W = kRagFwdWork > kRagBwdWork ? kRagFwdWork : kRagBwdWork;
  int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  lds_f* base = (lds_f*)smem;
  auto zero_fill = [&]() {
    const int total = (int)train_ragged_lds_floats(ly.n_blocks);
    for (int i = tid; i < total; i += nthr) base[i] = 0.f;
  };
  // length order: from the schedule workspace, or (srfrd_encoder_train_ranked) from the id plane itself - no launch in front
  const bool ranked = a.rank_G > 0 && a.B <= 512 * kRagChunks;
  RagT0 t0v;
  if (ranked) {
    t0v = rag_rank_batch(a.in_ids, a.B, (lds_i*)base, tid, zero_fill);
  } else {
    t0v = rag_load_t0(a, tid);
    zero_fill();
  }
  // pair stride of the length order; 0: workgroup x takes sequence x
  const int G = __builtin_amdgcn_readfirstlane(ranked ? a.rank_G : (rag_ordered(a) ? a.sched[kSchedG] : 0));
  RagFwdLds fm;
  fm.bXS = base;
  fm.bQN = base + LP * SLD;
  fm.bQ = fm.bQN + LP * DS;
  fm.bK = fm.bQ + LP * DS;
  fm.bV = fm.bK + LP * DS;
  lds_f* ftail = fm.bV + LP * DS;         // (the forward's per-row arrays: its over-reads behind bV stay in the allocation)
  fm.s_in = (lds_i*)ftail;
  fm.s_keep = ftail + LP;
  fm.s_pid = (lds_i*)(ftail + 2 * LP);
  fm.s_nid = (lds_i*)(ftail + 3 * LP);
  fm.s_misc = ftail + 4 * LP;
  static_assert(LP * SLD + 4 * LP * DS + 5 * LP == kRagFwdWork, "forward working set");
  // The hand-off (rag_seam_handoff): the forward's position-indexed x IS the backward's slot 0, and d hidden's slot lies inside
  // bQ and the unused rows in front of bK's position 0 - the one matrix the forward's head has no use for
  constexpr int oG = (kRagSH + kRagSeamG * 52) * DS;
  static_assert(oG >= LP * SLD + LP * DS && oG + 50 * DS <= LP * SLD + 2 * LP * DS + kRagSH * DS, "d hidden lands in dead floats");
  lds_f* s_ln = base + W;
  fm.s_ln = s_ln;
  const RagBwdLds bm{base, s_ln, s_ln + ln_cache_floats(ly.n_blocks)};
  __syncthreads();
  fill_ln_cache(s_ln, a.dense, ly);
  const uint32_t seed = a.seed_dev ? *a.seed_dev : a.seed;

  for (int iter = 0;; ++iter) {
    if (iter > 0) {                       // the previous backward's leftovers: the forward starts from zeros, as in its own launch
      for (int i = tid; i < W; i += nthr) base[i] = 0.f;
      __syncthreads();
    }
    const int x = (int)blockIdx.x + iter * (int)gridDim.x;      // rag_take, with the lengths and the stride found above
    const int take = x >= a.B ? -1 : (G > 0 ? rag_select(t0v, a.B, rag_want(x, G, a.B), (lds_i*)fm.bXS, tid) : x);
    const int b = __builtin_amdgcn_readfirstlane(take);
    if (b < 0) break;
    const RagSeam hs = rag_fwd_seq<K_, 1, DI_, true>(a, fm, b, tid, wave, seed);
    // (rag_fwd_seq ended with a workgroup barrier: its checkpoint stores are visible to every wave of the workgroup, and
    // nobody reads the forward's matrices any more)
    rag_seam_handoff<K_, DI_>(bm, hs, W, tid);
    __syncthreads();
    rag_bwd_seq<K_, DI_, RMW_, true>(a, bm, b, iter, tid, wave, seed, hs);
  }
}

int launch_train_ragged(const KernelPlan& k, const EncArgs& a, void* stream) {
  return with_variant_flag(k, [&](auto K, auto DI, auto rmw) { return launch_enc(encoder_train_ragged_kernel<K, DI, rmw>, k, stream, a); });
}

}  // namespace srfrd

using namespace srfrd;

// The step's scratch as srfrd_encoder_train_sched demands it: d hidden of every position, and SRFRN's logit gradients.  (The
// kernel handed these from its forward to its backward through this buffer; they stay in LDS now and nothing touches it,
// but the entry point's argument list and its refusals are pinned.)
extern "C" int64_t srfrd_train_scratch_floats(const srfrd_layout* lay, int B, int L) {
  if (!lay || B <= 0 || L <= 0) return 0;
  return (int64_t)B * L * (lay->d_out + (lay->kind == SRFRD_SRFRN ? 2 : 0));
}

extern "C" int srfrd_encoder_train_sched(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                                         const int64_t* input_ids, const int64_t* fake_ids, const int64_t* pos_ids,
                                         const int64_t* pos_fake, const int64_t* neg_ids, const int64_t* neg_fake, int B, int L,
                                         double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                                         float* hidden, float* pos_logits, float* neg_logits, float* save_x, float* save_h1,
                                         float* save_aux, float* loss_part, const float* d_hidden, const float* d_pos,
                                         const float* d_neg, int fused_bce, float* grad_table, float* table_contrib,
                                         float* grad_slabs, float* scratch, int64_t scratch_floats, const int32_t* sched,
                                         int sched_mode, void* stream) {
  if (!check_sched(sched, sched_mode)) return SRFRD_E_ARG;
  (void)d_pos; (void)d_neg;                  // (the kernel computes the logit gradients itself; a d_hidden makes the plan refuse)
  EncCall c = {};
  c.lay = lay; c.item_table = item_table; c.dense = dense; c.packed = packed; c.input_ids = input_ids; c.fake_ids = fake_ids;
  c.pos_ids = pos_ids; c.pos_fake = pos_fake; c.neg_ids = neg_ids; c.neg_fake = neg_fake; c.B = B; c.L = L; c.dropout_p = dropout_p;
  c.seed = seed; c.seed_dev = seed_dev; c.seq_index0 = seq_index0; c.hidden = hidden; c.pos_logits = pos_logits; c.neg_logits = neg_logits;
  c.save_x = save_x; c.save_h1 = save_h1; c.save_aux = save_aux; c.loss_part = loss_part;
  c.d_hidden = d_hidden; c.fused_bce = fused_bce; c.grad_table = grad_table; c.table_contrib = table_contrib; c.grad_slabs = grad_slabs;
  c.scratch = scratch; c.scratch_floats = scratch_floats; c.demand_scratch = true;
  c.sched = sched; c.sched_mode = sched_mode; c.stream = stream;
  return enc_run(c, kTrain);
}

// srfrd_encoder_train_sched without srfrd_seq_order in front of it: pair_stride > 0 asks for the length order of sched_mode 1
// and every workgroup ranks the batch from input_ids itself (rag_rank_batch); 0: no schedule.  No scratch: nothing reads it.
extern "C" int srfrd_encoder_train_ranked(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                                          const int64_t* input_ids, const int64_t* fake_ids, const int64_t* pos_ids,
                                          const int64_t* pos_fake, const int64_t* neg_ids, const int64_t* neg_fake, int B, int L,
                                          double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                                          float* hidden, float* pos_logits, float* neg_logits, float* save_x, float* save_h1,
                                          float* save_aux, float* loss_part, int fused_bce, float* grad_table,
                                          float* table_contrib, float* grad_slabs, int pair_stride, void* stream) {
  if (pair_stride < 0 || (reinterpret_cast<uintptr_t>(input_ids) & 15) != 0) return SRFRD_E_ARG;      // (the scan reads two ids per lane)
  EncCall c = {};
  c.lay = lay; c.item_table = item_table; c.dense = dense; c.packed = packed; c.input_ids = input_ids; c.fake_ids = fake_ids;
  c.pos_ids = pos_ids; c.pos_fake = pos_fake; c.neg_ids = neg_ids; c.neg_fake = neg_fake; c.B = B; c.L = L; c.dropout_p = dropout_p;
  c.seed = seed; c.seed_dev = seed_dev; c.seq_index0 = seq_index0; c.hidden = hidden; c.pos_logits = pos_logits; c.neg_logits = neg_logits;
  c.save_x = save_x; c.save_h1 = save_h1; c.save_aux = save_aux; c.loss_part = loss_part;
  c.fused_bce = fused_bce; c.grad_table = grad_table; c.table_contrib = table_contrib; c.grad_slabs = grad_slabs;
  c.rank_G = pair_stride; c.stream = stream;
  return enc_run(c, kTrain);
}
