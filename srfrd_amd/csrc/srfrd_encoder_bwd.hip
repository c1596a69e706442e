// Fused SRFRD encoder BACKWARD for MI355X (gfx950): per sequence, walks the blocks in reverse with the working set in
// LDS - LayerNorms recomputed from the forward's checkpoints, q / k / v, the attention probabilities (sign-coded with
// their dropout mask), the attention output and the FFN activation read back from them - back-propagates on the fp32
// matrix cores, scatters item-row gradients with float atomics and accumulates every dense-parameter gradient in a
// per-workgroup slab.  Replaces the autograd pass behind `loss.backward()` (reference trainer.py:40).
#include "srfrd_enc_common.h"

#include "srfrd_encoder_bwd_kernel.inc"

namespace srfrd {

int launch_bwd_first(const KernelPlan& k, const EncArgs& a, void* stream) {
  switch (k.form) {
    case kL50:
      if (k.variant < 0) return launch_enc(encoder_bwd_kernel<50, 64, 8, 50>, k, stream, a);
      return with_variant(k.variant, [&](auto v) {
        constexpr KindVariant kv = kKindVariants[decltype(v)::value];
        return with_flag(k.flag, [&](auto t) { return launch_enc(encoder_bwd_kernel<50, 64, 8, 50, kv.K, decltype(t)::value, kv.DI>, k, stream, a); });
      });
    case kLP64: return launch_enc(encoder_bwd_kernel<50, 64, 8>, k, stream, a);
    case kLP32: return launch_enc(encoder_bwd_kernel<50, 32, 8>, k, stream, a);
    default: return launch_enc(encoder_bwd_kernel<0, 0, 0>, k, stream, a);
  }
}

}  // namespace srfrd

using namespace srfrd;

extern "C" int srfrd_bwd_grid(const srfrd_layout* lay, int B, int L) {
  if (!lay || B <= 0 || L <= 0) return SRFRD_E_ARG;
  return bwd_grid(*lay, B, L, num_cu());
}

static int encoder_bwd_impl(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                            const int64_t* input_ids, const int64_t* fake_ids, const int64_t* pos_ids,
                            const int64_t* pos_fake, const int64_t* neg_ids, const int64_t* neg_fake, int B, int L,
                            double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                            const float* hidden, const float* pos_logits, const float* neg_logits,
                            const float* save_x, const float* save_h1, const float* save_aux, const float* d_hidden,
                            const float* d_pos,
                            const float* d_neg, int fused_bce, float* grad_table, float* table_contrib, float* grad_slabs,
                            float* scratch, int64_t scratch_floats, float* dbg, int dbg_seq, const int32_t* sched, int sched_mode,
                            void* stream) {
  const int sw = read_switches();
  EncArgs a = {};
  a.sched = sched_mode != 0 ? sched : nullptr;
  a.sched_mode = a.sched ? sched_mode : 0;
  a.ragged_off = (sw & SRFRD_SW_RAGGED_FULL_ROWS) != 0;
  int rc = fill_args(a, lay, item_table, dense, packed, input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, B, L,
                     dropout_p, seed, seed_dev, seq_index0);
  if (rc) return rc;
  if (!hidden || !save_x || !save_h1 || !save_aux || !grad_table || !grad_slabs) return SRFRD_E_ARG;
  if (fused_bce && !(pos_ids && neg_ids && pos_logits && neg_logits)) return SRFRD_E_ARG;
  a.c_hidden = hidden; a.c_pl = pos_logits; a.c_nl = neg_logits; a.c_save_x = save_x; a.c_save_h1 = save_h1; a.c_save_aux = save_aux;
  a.d_hidden = d_hidden; a.d_pos = d_pos; a.d_neg = d_neg; a.fused_bce = fused_bce;
  a.grad_table = grad_table; a.grad_slabs = grad_slabs; a.contrib = table_contrib;
  a.dbg = dbg; a.dbg_seq = dbg_seq;
  srfrd_debug_shape(lay, L, &a.dbg_slot, nullptr);
  int mode = (pos_ids ? SRFRD_PLAN_POS : 0) | (neg_ids ? SRFRD_PLAN_NEG : 0) | (fused_bce && !d_hidden ? SRFRD_PLAN_FUSED_BCE : 0) |
             (dropout_p > 0.0 ? SRFRD_PLAN_DROPOUT : 0);
#ifndef SRFRD_STAMPS
  if (dbg) mode |= SRFRD_PLAN_TAPS;            // (diagnostic build: `dbg` receives the phase stamps, not taps)
#endif
  const KernelPlan k = encoder_plan(*lay, B, L, mode, sw, num_cu(), scratch ? scratch_floats : 0).bwd;
  if (k.rc) return k.rc;
  if (k.scratch_stride) {
    a.scratch = scratch;
    a.scratch_stride = k.scratch_stride;
  }
  switch (k.family) {
    case kBwdRagged: return launch_bwd_ragged(k, a, stream);
    case kBwdSlots: return launch_bwd_slots(k, a, stream);
    case kBwdChunks: return launch_bwd_chunks(k, a, stream);
    case kBwdLong: return launch_bwd_long(k, &a, stream);
    default: return launch_bwd_first(k, a, stream);
  }
}

extern "C" int srfrd_encoder_bwd(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                                 const int64_t* input_ids, const int64_t* fake_ids, const int64_t* pos_ids,
                                 const int64_t* pos_fake, const int64_t* neg_ids, const int64_t* neg_fake, int B, int L,
                                 double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                                 const float* hidden, const float* pos_logits, const float* neg_logits,
                                 const float* save_x, const float* save_h1, const float* save_aux, const float* d_hidden,
                                 const float* d_pos,
                                 const float* d_neg, int fused_bce, float* grad_table, float* table_contrib, float* grad_slabs,
                                 float* scratch, int64_t scratch_floats, float* dbg, int dbg_seq, void* stream) {
  return encoder_bwd_impl(lay, item_table, dense, packed, input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, B, L, dropout_p,
                          seed, seed_dev, seq_index0, hidden, pos_logits, neg_logits, save_x, save_h1, save_aux, d_hidden, d_pos,
                          d_neg, fused_bce, grad_table, table_contrib, grad_slabs, scratch, scratch_floats, dbg, dbg_seq, nullptr, 0,
                          stream);
}

extern "C" int srfrd_encoder_bwd_sched(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                                       const int64_t* input_ids, const int64_t* fake_ids, const int64_t* pos_ids,
                                       const int64_t* pos_fake, const int64_t* neg_ids, const int64_t* neg_fake, int B, int L,
                                       double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                                       const float* hidden, const float* pos_logits, const float* neg_logits,
                                       const float* save_x, const float* save_h1, const float* save_aux, const float* d_hidden,
                                       const float* d_pos, const float* d_neg, int fused_bce, float* grad_table,
                                       float* table_contrib, float* grad_slabs, float* scratch, int64_t scratch_floats,
                                       const int32_t* sched, int sched_mode, void* stream) {
  if (sched_mode < 0 || sched_mode > 1 || (sched_mode != 0 && !sched)) return SRFRD_E_ARG;
  return encoder_bwd_impl(lay, item_table, dense, packed, input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, B, L, dropout_p,
                          seed, seed_dev, seq_index0, hidden, pos_logits, neg_logits, save_x, save_h1, save_aux, d_hidden, d_pos,
                          d_neg, fused_bce, grad_table, table_contrib, grad_slabs, scratch, scratch_floats, nullptr, 0, sched,
                          sched_mode, stream);
}

