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
      return with_variant_flag(k, [&](auto K, auto DI, auto t) { return launch_enc(encoder_bwd_kernel<50, 64, 8, 50, K, t, DI>, k, stream, a); });
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

// the forward's outputs as an EncCall names them: the backward pass only reads them (EncArgs::c_*)
static float* rd(const float* p) { return const_cast<float*>(p); }

extern "C" int srfrd_encoder_bwd(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                                 const int64_t* input_ids, const int64_t* fake_ids, const int64_t* pos_ids,
                                 const int64_t* pos_fake, const int64_t* neg_ids, const int64_t* neg_fake, int B, int L,
                                 double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                                 const float* hidden, const float* pos_logits, const float* neg_logits,
                                 const float* save_x, const float* save_h1, const float* save_aux, const float* d_hidden,
                                 const float* d_pos, const float* d_neg, int fused_bce, float* grad_table, float* table_contrib,
                                 float* grad_slabs, float* scratch, int64_t scratch_floats, float* dbg, int dbg_seq, void* stream) {
  EncCall c = {};
  c.lay = lay; c.item_table = item_table; c.dense = dense; c.packed = packed; c.input_ids = input_ids; c.fake_ids = fake_ids;
  c.pos_ids = pos_ids; c.pos_fake = pos_fake; c.neg_ids = neg_ids; c.neg_fake = neg_fake; c.B = B; c.L = L; c.dropout_p = dropout_p;
  c.seed = seed; c.seed_dev = seed_dev; c.seq_index0 = seq_index0;
  c.hidden = rd(hidden); c.pos_logits = rd(pos_logits); c.neg_logits = rd(neg_logits);
  c.save_x = rd(save_x); c.save_h1 = rd(save_h1); c.save_aux = rd(save_aux);
  c.d_hidden = d_hidden; c.d_pos = d_pos; c.d_neg = d_neg; c.fused_bce = fused_bce;
  c.grad_table = grad_table; c.table_contrib = table_contrib; c.grad_slabs = grad_slabs;
  c.scratch = scratch; c.scratch_floats = scratch_floats; c.dbg = dbg; c.dbg_seq = dbg_seq; c.stream = stream;
  return enc_run(c, kBackward);
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
  if (!check_sched(sched, sched_mode)) return SRFRD_E_ARG;
  EncCall c = {};
  c.lay = lay; c.item_table = item_table; c.dense = dense; c.packed = packed; c.input_ids = input_ids; c.fake_ids = fake_ids;
  c.pos_ids = pos_ids; c.pos_fake = pos_fake; c.neg_ids = neg_ids; c.neg_fake = neg_fake; c.B = B; c.L = L; c.dropout_p = dropout_p;
  c.seed = seed; c.seed_dev = seed_dev; c.seq_index0 = seq_index0;
  c.hidden = rd(hidden); c.pos_logits = rd(pos_logits); c.neg_logits = rd(neg_logits);
  c.save_x = rd(save_x); c.save_h1 = rd(save_h1); c.save_aux = rd(save_aux);
  c.d_hidden = d_hidden; c.d_pos = d_pos; c.d_neg = d_neg; c.fused_bce = fused_bce;
  c.grad_table = grad_table; c.table_contrib = table_contrib; c.grad_slabs = grad_slabs;
  c.scratch = scratch; c.scratch_floats = scratch_floats; c.sched = sched; c.sched_mode = sched_mode; c.stream = stream;
  return enc_run(c, kBackward);
}

