/*
 * srfrd_hip.h  --  C ABI of libsrfrd_hip.so, the MI355X (gfx950) implementation of the SRFRD hot path.
 *
 * The reference (oss0430/SRFRD) has no FFI: its hot path is the Python nn.Module API
 * `model(user_ids, input_ids, fake_ids, positive_ids, positive_fake_ids, negative_ids, negative_fake_ids)`
 * (reference SRFR_model.py:92, :192, :473, :651), `model.predict(...)` (:144, :241, :532, :668) and the
 * train step of reference trainer.py:27-41.  Every device operation those calls perform in stock torch
 * ops is replaced by the launchers below; `srfrd_amd/` (Python) keeps the reference's module / state_dict
 * surface on top of them (see INTEGRATION.md for the binding a reference maintainer would add).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked [host];
 *  - the caller owns every buffer; launchers only enqueue work on `stream` (hipStream_t passed as void*) and never
 *    allocate or synchronise => graph-capturable.  The only process-wide state is a mutex-protected cache of per-device
 *    facts (CU count, which kernels already have their > 64 KiB dynamic-LDS opt-in on which device), so launchers may
 *    be called from several host threads and for several devices of one process;
 *  - return value: 0 = ok, < 0 = argument / capability error (SRFRD_E_*), > 0 = hipError_t of the launch;
 *  - ids are int64 (torch LongTensor, reference trainer.py:29), row-major (B, L), left-padded with 0;
 *  - all floating-point data is fp32 (dtype "f32"); integer label / rank work is exact.
 */
#ifndef SRFRD_HIP_H
#define SRFRD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRFRD_MAX_BLOCKS 8
#define SRFRD_MAX_D 64          /* hidden width limit of the fused kernels (one lane per channel) */

enum srfrd_kind {               /* reference classes, SRFR_model.py */
  SRFRD_SASREC = 0,             /* :572 */
  SRFRD_SRFR = 1,               /* :53  */
  SRFRD_SRFRN = 2,              /* :154 */
  SRFRD_SRFU_B = 3,             /* :543 */
  SRFRD_SRFU_F = 4,             /* :553 */
  SRFRD_SRFU_R = 5              /* :562 */
};

enum srfrd_error {
  SRFRD_E_ARG = -1,             /* bad argument (null pointer, size out of range) */
  SRFRD_E_UNSUPPORTED = -2,     /* configuration outside what the fused kernels cover (D > 64, L too long for LDS and no scratch given) */
  SRFRD_E_DEVICE = -3           /* not a gfx950 device / LDS attribute could not be set */
};

/* Per-block element offsets into the dense parameter vector (SURVEY Appendix B names in comments). */
typedef struct srfrd_block_off {
  int64_t ln1_w, ln1_b;         /* attention_layernorms.i.{weight,bias}          (D)      */
  int64_t in_w, in_b;           /* attention_layers.i.in_proj_{weight,bias}      (3D,D),(3D) */
  int64_t out_w, out_b;         /* attention_layers.i.out_proj.{weight,bias}     (D,D),(D) */
  int64_t ln2_w, ln2_b;         /* forward_layernorms.i.{weight,bias}            (D)      */
  int64_t c1_w, c1_b;           /* forward_layers.i.conv1.{weight,bias}          (D,D,1),(D) */
  int64_t c2_w, c2_b;           /* forward_layers.i.conv2.{weight,bias}          (D,D,1),(D) */
} srfrd_block_off;

/*
 * Model geometry + the canonical layout of the "dense" parameter vector: every parameter except the item
 * table, concatenated in this order.  The same offsets index the parameters, a dense-gradient slab and the
 * Adam moments, so one descriptor serves forward, backward, reduce and optimizer.
 */
typedef struct srfrd_layout {
  int32_t kind, n_items, max_len, d_item, d_fake, D, d_out, n_labels, n_blocks, n_heads;
  int32_t side_rows, side_cols; /* fake_embed (3,d_fake) | user_label_embed (n_labels,D) | none (0,0) */
  int32_t table_bf16;           /* 0: every `item_table` argument is the fp32 parameter (n_items+1, d_item).  1: it is the
                                   bf16 SHADOW of it (uint16_t, same shape; BASELINE configs[1] / [4] "bf16" table): the
                                   forward / backward / ranking GATHERS read half the bytes; gradients, the fp32 master
                                   and Adam are unchanged (the optimizer launchers rewrite the shadow) */
  int32_t flags;                /* SRFRD_LAYOUT_* bits; srfrd_layout_init writes 0.  A layout with a bit outside the ones defined
                                   below is refused: the plan queries and every encoder entry point answer
                                   SRFRD_E_UNSUPPORTED before any launch.  Ranking, the loss heads and the optimizer do not read it.
                                   SRFRD_LAYOUT_MASK_PAD_KEYS: the LEADING pads of a sequence leave its attention keys (the
                                   original SASRec's key-padding mask; the reference passes none, SRFR_model.py:112).  With
                                   t0(b) = the index of the first non-zero id of input_ids[b] (L if there is none):
                                    - a live query row r >= t0 has P[r, j] = softmax_j(s[r, j]) over t0 <= j <= r; keys j < t0 get an
                                      exact 0 and take no part in the row maximum;
                                    - only the leading pads are masked: an id 0 at a position >= t0 stays a key, as without the flag;
                                    - pad query rows r < t0 produce the zero outputs they produce without the flag (their internal
                                      values are unspecified but finite); a sequence of pads gives zeros and no NaN;
                                    - attention-dropout masks keep their (row, col) coordinates; embedding, LayerNorms, FFN, heads,
                                      logits and the BCE partial sums are unchanged;
                                    - the backward is the gradient of the above: dk / dv of a leading pad are exact zeros, so the
                                      key / value biases lose those terms;
                                    - flag off, or a batch without pads: the results without the flag, bit for bit. */
  int64_t off_pos;             /* pos_embed / pos_emb                  (max_len, d_item) */
  int64_t off_side;             /* fake_embed / user_label_embed        (side_rows, side_cols) */
  srfrd_block_off blk[SRFRD_MAX_BLOCKS];
  int64_t off_lc_w, off_lc_b;   /* last_conv.{weight,bias}  (d_item,D,1),(d_item)   SRFR only, else -1 */
  int64_t off_ll_w, off_ll_b;   /* last_layernorm.{weight,bias}         (d_out) */
  int64_t n_dense;              /* elements in the dense vector */
  int64_t n_table;              /* (n_items + 1) * d_item */
} srfrd_layout;
#define SRFRD_LAYOUT_MASK_PAD_KEYS 1     /* srfrd_layout::flags: see there */

/* [host] fills `lay`; replaces the per-class constructors' shape logic (reference SRFR_model.py:54-90, 155-190,
 * 431-466, 573-615).  n_blocks outside 1 .. SRFRD_MAX_BLOCKS -> SRFRD_E_ARG: the backward kernels prefetch the checkpoints of
 * block n_blocks - 1 before their loop, so a model without blocks is refused here, not run. */
int srfrd_layout_init(srfrd_layout* lay, int kind, int n_items, int max_len, int d_item, int d_fake,
                      int n_labels, int n_blocks, int n_heads);

/* [host] capability query: dynamic LDS bytes the first-generation fused forward / backward kernels need for sequence
 * length L (0 if that working set does not fit the 160 KiB LDS of a gfx950 CU: such shapes run the long-sequence kernels -
 * LDS-resident for hidden width 50 up to L = 208, a global-scratch build beyond - and need srfrd_scratch_floats). */
int srfrd_lds_bytes(const srfrd_layout* lay, int L, int64_t* fwd_bytes, int64_t* bwd_bytes);

/* [host] floats of global scratch the forward / backward need for (B, L): 0 when the first-generation working set fits
 * LDS; otherwise one slice per workgroup: the long-sequence kernels keep what crosses their passes there (the row-chunked
 * backward: three [L][D] intermediates), the global-scratch build its whole working set - every shape runs on the GPU. */
int srfrd_scratch_floats(const srfrd_layout* lay, int B, int L, int64_t* fwd_floats, int64_t* bwd_floats);

/* [host] floats of the forward's `save_aux` checkpoint buffer for (B, L): per block and sequence the FFN hidden
 * activation relu(drop(.)), the attention output P v, the scaled queries, the keys and the values (L, D each) and the
 * attention probabilities (n_heads, L, LP = L rounded up to 16), the latter sign-coded with the attention-dropout mask (a
 * dropped entry is stored negated); sequence-major (all blocks of one sequence are contiguous). */
int64_t srfrd_aux_floats(const srfrd_layout* lay, int B, int L);

/* [host] number of persistent workgroups the backward launches for batch B at sequence length L (= rows of `grad_slabs`):
 * a function of the layout and the shape only. */
int srfrd_bwd_grid(const srfrd_layout* lay, int B, int L);

/* [host] the encoder's kernel plan, asked without a GPU: which instantiation srfrd_encoder_fwd(_sched, _last) and
 * srfrd_encoder_bwd(_sched) launch for (lay, B, L) in `mode` (SRFRD_PLAN_* bits: what the call computes) under `switches`
 * (SRFRD_SW_* bits: the environment switches of the same names, which the launchers read on every call), on a device with
 * n_cu CUs, given scratch_floats of caller scratch (0: none).  For each direction, writes the instantiation's name as a
 * kernel trace prints it, without spaces ("srfrd::encoder_fwd_ragged_kernel<0,1,50>"; at most name_len bytes with the NUL)
 * and grids[0] (forward) / grids[1] (backward): the workgroup count, or SRFRD_E_UNSUPPORTED with an empty name where that
 * call returns SRFRD_E_UNSUPPORTED.  Returns 0 or SRFRD_E_ARG. */
#define SRFRD_PLAN_POS 1          /* positive target ids given (pos_logits) */
#define SRFRD_PLAN_NEG 2          /* negative target ids given (neg_logits) */
#define SRFRD_PLAN_CKPT 4         /* forward: training checkpoints written (save_x / save_h1 / save_aux) */
#define SRFRD_PLAN_LOSS 8         /* forward: BCE partial sums written (loss_part) */
#define SRFRD_PLAN_DROPOUT 16     /* dropout_p > 0 */
#define SRFRD_PLAN_FUSED_BCE 32   /* backward: fused BCE gradient (fused_bce set, d_hidden NULL) */
#define SRFRD_PLAN_TAPS 64        /* debug taps (dbg != NULL) */
#define SRFRD_SW_GENERIC 1        /* the run-time-geometry instantiation for every shape the LDS holds */
#define SRFRD_SW_NO_RAGGED 2      /* not the ragged pair at seq_len 50 */
#define SRFRD_SW_RAGGED_FULL_ROWS 4   /* the ragged pair computes every row (same kernels) */
#define SRFRD_SW_NO_SLOTS50 8     /* not the slot-placed backward at seq_len 50 (nor the ragged pair) */
#define SRFRD_SW_NO_SLOTS 16      /* long sequences: neither the slot-placed nor the row-chunked backward */
#define SRFRD_SW_NO_ROWS 32       /* long sequences: not the row-owner forward */
#define SRFRD_SW_ROWS_ALWAYS 64   /* the row-owner forward wherever it serves (and not the ragged pair) */
#define SRFRD_SW_TOPK_FP32 128    /* ranking: the fp32 stream wherever the bf16 matrix-core stream would serve (the encoder ignores it) */
int srfrd_encoder_plan(const srfrd_layout* lay, int B, int L, int mode, int switches, int n_cu, int64_t scratch_floats,
                       char* fwd_name, char* bwd_name, int name_len, int32_t* grids);
/* [host] the train direction of the same plan: the instantiation srfrd_encoder_train_sched launches for (lay, B, L, mode,
 * switches, n_cu, scratch_floats) - its name in `name` and its workgroup count in *grid - or SRFRD_E_UNSUPPORTED in *grid
 * with an empty name where that call refuses.  Returns 0 or SRFRD_E_ARG. */
int srfrd_encoder_plan_train(const srfrd_layout* lay, int B, int L, int mode, int switches, int n_cu, int64_t scratch_floats,
                             char* name, int name_len, int32_t* grid);

/* [host] floats per debug-tap slot and number of slots (tests only). */
int srfrd_debug_shape(const srfrd_layout* lay, int L, int64_t* slot_floats, int32_t* n_slots);

/*
 * Weight packing.  The fused kernels read every (out, in) weight matrix of the encoder (in_proj's three slices,
 * out_proj, conv1, conv2, last_conv) from `packed`: a copy pre-swizzled into v_mfma_f32_16x16x4_f32 B-fragment order
 * in both product forms (x W^T for the forward, dy W for the backward).  Call after every parameter update and before
 * srfrd_encoder_fwd / _bwd.  packed holds srfrd_packed_floats(lay) floats.  If `state` != NULL the same launch also
 * performs srfrd_step_begin's advance for the NEXT step (the fused train step ends with this launch), else lr / betas
 * are ignored.
 */
int64_t srfrd_packed_floats(const srfrd_layout* lay);
int srfrd_pack_weights(const srfrd_layout* lay, const float* dense, float* packed,
                       uint32_t* state, double lr, double beta1, double beta2, void* stream);

/*
 * Fused forward: embedding gather (+pos, +fake / user-label channel, pad mask), n_blocks x
 * {LN -> causal self-attention -> +res -> LN -> PW-FFN -> mask}, (last_conv), last LN, pos/neg logits and the
 * masked-BCE partial sums.  Replaces reference SRFR_model.py:92-142 (and the SRFRN / SRFU / SASRec twins)
 * plus the loss terms of reference trainer.py:36-38.
 *
 *  item_table (n_items+1, d_item) fp32 - or its bf16 shadow when lay->table_bf16 -, dense (n_dense) parameters;
 *    packed: srfrd_pack_weights(dense)
 *  input_ids, fake_ids (B,L); fake_ids may be NULL (SASRec ignores it; SRFR/SRFRN treat NULL as all-zero,
 *    reference SRFR_model.py:27-28)
 *  pos_ids/neg_ids (B,L) or NULL (no logits, reference :126-136); pos_fake/neg_fake used by SRFRN only
 *  dropout_p > 0 selects train mode; masks come from the counter hash of srfrd_rng.h keyed by
 *    (seed, site, seq_index0 + b, row, col); if seed_dev != NULL the seed is read from device memory
 *  hidden (B,L,d_out), pos_logits/neg_logits (B,L) outputs (logit pointers may be NULL iff the id pointer is)
 *  save_x (B, n_blocks+1, L, D): block inputs and the last block's output; save_h1 (B, n_blocks, L, D):
 *    post-attention residual; save_aux: srfrd_aux_floats() floats (see there); all three NULL for inference.
 *    Sequence-major and opaque to the caller: written here, read back by srfrd_encoder_bwd
 *  loss_part (B,3) or NULL: per sequence {sum softplus(-pos), sum softplus(neg), count} over pos_ids != 0
 *  scratch / scratch_floats: srfrd_scratch_floats() floats of workspace (NULL / 0 when that is 0)
 *  dbg / dbg_seq: debug taps of one sequence (tests only; NULL otherwise)
 */
int srfrd_encoder_fwd(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                      const int64_t* input_ids, const int64_t* fake_ids,
                      const int64_t* pos_ids, const int64_t* pos_fake,
                      const int64_t* neg_ids, const int64_t* neg_fake,
                      int B, int L, double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                      float* hidden, float* pos_logits, float* neg_logits,
                      float* save_x, float* save_h1, float* save_aux, float* loss_part,
                      float* scratch, int64_t scratch_floats,
                      float* dbg, int dbg_seq, void* stream);

/*
 * Sequence -> workgroup schedule of the seq_len-50 ("ragged") encoder kernels.  At the reference's default geometry
 * (hidden 50, maxlen 50: trainer.py:123-129) srfrd_encoder_fwd / _bwd compute only the rows a left-padded sequence really
 * has, so a launch is as slow as its slowest CU - two workgroups share a CU, and a long sequence should share it with a
 * short one.  srfrd_seq_order (one small launch per batch) writes every sequence's first non-pad position into `sched`
 * (int32[srfrd_sched_ints(B)], caller-owned, valid for THIS batch's input_ids only); the _sched forms of the encoder entry
 * points take it:
 *   sched_mode 0  no schedule (== srfrd_encoder_fwd / _bwd: workgroup x takes sequences x, x + grid, ...)
 *   sched_mode 1  length order: workgroup x takes the sequence of rank perm(x) (longest first, ties by index), perm = the
 *                 `pair_stride` longest first, then the shortest ascending (the workgroup that joins the longest sequence's
 *                 CU brings the shortest), the rest descending; every workgroup selects its sequence from the B lengths
 *                 itself (no sort launch)
 * Results never depend on the schedule beyond the summation order of the per-workgroup dense-gradient slabs, which is a
 * function of the batch.  Other geometries ignore the schedule.
 * Reference counterpart: none (the reference runs stock torch ops over the full padded batch, SRFR_model.py:92-142).
 */
int64_t srfrd_sched_ints(int B);
int srfrd_seq_order(const int64_t* input_ids, int B, int L, int pair_stride, int32_t* sched, void* stream);
int srfrd_encoder_fwd_sched(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                            const int64_t* input_ids, const int64_t* fake_ids,
                            const int64_t* pos_ids, const int64_t* pos_fake,
                            const int64_t* neg_ids, const int64_t* neg_fake,
                            int B, int L, double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                            float* hidden, float* pos_logits, float* neg_logits,
                            float* save_x, float* save_h1, float* save_aux, float* loss_part,
                            float* scratch, int64_t scratch_floats,
                            const int32_t* sched, int sched_mode, void* stream);
int srfrd_encoder_bwd_sched(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                            const int64_t* input_ids, const int64_t* fake_ids,
                            const int64_t* pos_ids, const int64_t* pos_fake,
                            const int64_t* neg_ids, const int64_t* neg_fake,
                            int B, int L, double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                            const float* hidden, const float* pos_logits, const float* neg_logits,
                            const float* save_x, const float* save_h1, const float* save_aux,
                            const float* d_hidden, const float* d_pos, const float* d_neg, int fused_bce,
                            float* grad_table, float* table_contrib, float* grad_slabs,
                            float* scratch, int64_t scratch_floats,
                            const int32_t* sched, int sched_mode, void* stream);

/* [device] one fused training step's encoder work as ONE launch: srfrd_encoder_fwd_sched (training: targets, checkpoints, loss
 * partials) followed by srfrd_encoder_bwd_sched (fused BCE gradient) with the same arguments, each workgroup running a
 * sequence's forward and then its backward.  Arguments: the union of the two calls' (hidden / pos_logits / neg_logits /
 * save_* are written and read back); results are those of the two calls bit for bit.  Where the kernel plan has no train
 * kernel for the call (srfrd_encoder_plan_train: where the ragged seq_len-50 pair serves a call with SRFRD_PLAN_POS, _NEG,
 * _CKPT, _LOSS and _FUSED_BCE, dropout or not), returns SRFRD_E_UNSUPPORTED and launches nothing: make the two calls instead.
 * scratch: srfrd_train_scratch_floats(lay, B, L) floats or more (SRFRD_E_ARG otherwise) - where a workgroup's forward leaves
 * the head's hidden-state gradient for its backward; contents are of no use to the caller. */
int64_t srfrd_train_scratch_floats(const srfrd_layout* lay, int B, int L);
int srfrd_encoder_train_sched(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                              const int64_t* input_ids, const int64_t* fake_ids,
                              const int64_t* pos_ids, const int64_t* pos_fake,
                              const int64_t* neg_ids, const int64_t* neg_fake,
                              int B, int L, double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                              float* hidden, float* pos_logits, float* neg_logits,
                              float* save_x, float* save_h1, float* save_aux, float* loss_part,
                              const float* d_hidden, const float* d_pos, const float* d_neg, int fused_bce,
                              float* grad_table, float* table_contrib, float* grad_slabs,
                              float* scratch, int64_t scratch_floats,
                              const int32_t* sched, int sched_mode, void* stream);
/* [device] srfrd_encoder_train_sched for the fused BCE step WITHOUT srfrd_seq_order in front of it and without its workspace:
 * pair_stride > 0 asks for the length order of sched_mode 1 with that stride, and every workgroup finds the batch's first
 * non-pad positions from input_ids itself, as its first instructions (B <= 1024; larger batches: no schedule, as there);
 * pair_stride 0: no schedule; < 0, or input_ids not 16-byte aligned: SRFRD_E_ARG.  The same sequence -> workgroup assignment as srfrd_seq_order +
 * srfrd_encoder_train_sched, so the same results bit for bit.  Takes no scratch (the kernel has not read it since the
 * forward -> backward hand-off stays on chip) and no upstream gradients: fused_bce as there. */
int srfrd_encoder_train_ranked(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                               const int64_t* input_ids, const int64_t* fake_ids,
                               const int64_t* pos_ids, const int64_t* pos_fake,
                               const int64_t* neg_ids, const int64_t* neg_fake,
                               int B, int L, double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                               float* hidden, float* pos_logits, float* neg_logits,
                               float* save_x, float* save_h1, float* save_aux, float* loss_part,
                               int fused_bce, float* grad_table, float* table_contrib, float* grad_slabs,
                               int pair_stride, void* stream);

/* Inference forward for ranking: the encoder state of the LAST position only, hidden_last (B, d_out) - what the reference's
 * predict() takes from log2feats (SRFR_model.py:668-681: `log_feats[:, -1, :]`).  Same arithmetic as srfrd_encoder_fwd in
 * eval mode (row L - 1 of its `hidden`, bit for bit); the last block computes queries, attention rows, output projection
 * and FFN for the one 16-row tile holding that position.  Feed it to srfrd_predict_logits / srfrd_logits_topk with L = 1. */
int srfrd_encoder_fwd_last(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                           const int64_t* input_ids, const int64_t* fake_ids, int B, int L, float* hidden_last,
                           float* scratch, int64_t scratch_floats, void* stream);

/*
 * Fused backward of srfrd_encoder_fwd: LayerNorms are recomputed in LDS from save_x / save_h1; q / k / v, the FFN hidden
 * activation, the attention probabilities (with their dropout mask) and the attention output are read back from
 * save_aux.  Replaces the
 * autograd pass behind `loss.backward()` (reference trainer.py:40).
 *
 *  fused_bce != 0: d(pos_logits) = (sigmoid(pos)-1)[pos_ids!=0], d(neg_logits) = sigmoid(neg)[pos_ids!=0]
 *    (SUM reduction: the 1/count of the two means is applied by srfrd_adam_step via `stats`), d_hidden = 0;
 *  fused_bce == 0: upstream gradients d_hidden (B,L,d_out) / d_pos / d_neg (B,L) are read (each may be NULL).
 *  grad_table (n_items+1, d_item): += by float atomics (caller zeroes it; row 0 never written: padding_idx)
 *  table_contrib: NULL, or (3, B, L, d_item) floats for the DETERMINISTIC item-table scatter: instead of the atomics every
 *    (target kind {pos, neg, input}, sequence, position) writes its row contribution here (zeros where it has none) and
 *    srfrd_table_reduce sums the rows of each item in a fixed order into grad_table (bitwise reproducible)
 *  grad_slabs (srfrd_bwd_grid(lay, B, L), n_dense): per-workgroup partial dense gradients (fully overwritten)
 */
int srfrd_encoder_bwd(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                      const int64_t* input_ids, const int64_t* fake_ids,
                      const int64_t* pos_ids, const int64_t* pos_fake,
                      const int64_t* neg_ids, const int64_t* neg_fake,
                      int B, int L, double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                      const float* hidden, const float* pos_logits, const float* neg_logits,
                      const float* save_x, const float* save_h1, const float* save_aux,
                      const float* d_hidden, const float* d_pos, const float* d_neg, int fused_bce,
                      float* grad_table, float* table_contrib, float* grad_slabs,
                      float* scratch, int64_t scratch_floats,
                      float* dbg, int dbg_seq, void* stream);

/*
 * Deterministic item-table scatter, second half (the first is srfrd_encoder_bwd with table_contrib): n = 3 * B * L keys
 * (the item id each contribution row belongs to: pos ids, neg ids, input ids, in table_contrib's row order) sorted
 * ascending by a STABLE sort, with `order[i]` = the contribution row that sorted position i came from.  One wave per
 * run of equal keys adds that item's rows in sorted order and stores the sum to grad_table[key] (key 0 = padding_idx is
 * skipped; rows without contributions are not touched: the caller keeps them zero).  The summation order is a function
 * of the ids alone => the table gradient is bitwise reproducible, unlike the float-atomic form.
 */
int srfrd_table_reduce(const int64_t* sorted_keys, const int64_t* order, const float* table_contrib, int64_t n, int d_item,
                       float* grad_table, void* stream);

/* Sums the per-workgroup slabs into grad_dense (n_dense) in a fixed order (bitwise reproducible) and, if
 * loss_part != NULL, reduces it into stats[0..3] = {sum softplus(-pos), sum softplus(neg), count, 0}; with loss_out != NULL
 * (single rank: stats are already global) it also writes the loss, making srfrd_loss_finalize unnecessary. */
int srfrd_reduce_dense(const float* grad_slabs, int n_slabs, int64_t n_dense, float* grad_dense,
                       const float* loss_part, int B, float* stats, float* loss_out, void* stream);

/* The loss half of srfrd_reduce_dense on its own: stats[0..3] = {sum softplus(-pos), sum softplus(neg), count, 0} from the
 * forward's loss_part (B,3); loss_out (may be NULL) = the loss of these statistics.  The data-parallel step runs it right
 * after the forward so that the 16-byte all-reduce of the statistics overlaps the backward kernel. */
int srfrd_loss_stats(const float* loss_part, int B, float* stats, float* loss_out, void* stream);

/*
 * Optimizer state advance (one thread): t += 1, step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t)
 * (double precision, as torch.optim.Adam computes them on the host), next dropout seed.
 *  state: uint32[32] {t, base_seed, step_seed, -, float step_size, float bc2_sqrt, ticket root, -, 16 ticket shards, -...}
 *         (words 6 and 8..23 are the hand-off counters of srfrd_adam_pack_step, zero between launches; callers that
 *         never use that entry point may pass 8 words; words 3 and 7 are written by srfrd_step_begin_sched only, below)
 */
int srfrd_step_begin(uint32_t* state, double lr, double beta1, double beta2, void* stream);

/*
 * Dense Adam over the flat vector [table | dense] (torch.optim.Adam semantics, reference trainer.py:41, :390):
 *   g = grad[i] * gscale;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= step_size * m / (sqrt(v)/bc2_sqrt + eps)
 * gscale = 1 / stats[2] if stats != NULL (mean over non-pad targets, trainer.py:36-38) else 1.
 * The first n_zero gradient elements (the table, accumulated by atomics) are re-zeroed in the same pass.
 * [i0, i1) = the slice this rank updates (sharded optimizer); pass 0, n for all.  i0 is a multiple of 4 unless the slice
 * is empty (an empty slice launches nothing).
 * table_bf16 (may be NULL): bf16 shadow of the first n_table parameters (the item table); stepped elements below n_table
 * are also written there, rounded to nearest even.
 */
int srfrd_adam_step(float* param, float* grad, float* m, float* v, int64_t n, int64_t i0, int64_t i1,
                    int64_t n_zero, double beta1, double beta2, double eps,
                    const uint32_t* state, const float* stats, uint16_t* table_bf16, int64_t n_table, void* stream);

/*
 * Fused tail of the train step: srfrd_adam_step over the whole flat vector [table | pad | dense] (n floats, the dense
 * part starting at n_table_pad), the stepped encoder weights written straight into `packed` in both fragment forms
 * (what srfrd_pack_weights(dense) would produce; `packed` must have been packed once before), and the optimizer-state
 * advance of srfrd_step_begin for the NEXT step, done by the last block to finish; table_bf16 (may be NULL) = the bf16 shadow
 * of the item table (lay->n_table elements), rewritten with the stepped rows in the same pass.  `state` holds 32 words here:
 * state[6] and state[8..23] are the ticket counters of that hand-off (zero between launches).  Replaces optimizer.step() of reference trainer.py:41.
 */
int srfrd_adam_pack_step(const srfrd_layout* lay, float* param, float* grad, float* m, float* v, int64_t n,
                         int64_t n_table_pad, int64_t n_zero, double lr, double beta1, double beta2, double eps,
                         uint32_t* state, const float* stats, float* packed, uint16_t* table_bf16, void* stream);

/*
 * Learning-rate schedule, decoupled weight decay and gradient-norm clipping for the two Adam entry points above (DESIGN
 * section 19).  The schedule lives on the device, beside the step counter: a captured graph holds `opts` as a constant
 * and only t varies from replay to replay.
 *
 * THE formula (srfrd_amd.lr_at is its host mirror): for the 1-based step t, lr_t = lr * f(t), in double precision, with
 * w = warmup_steps, T = total_steps, r = final_ratio:
 *   t <= w :  f = t / w
 *   else   :  u = min(1, (t - w) / max(1, T - w)), and
 *             SRFRD_SCHED_CONSTANT  f = 1
 *             SRFRD_SCHED_LINEAR    f = 1 - (1 - r) u
 *             SRFRD_SCHED_COSINE    f = r + (1 - r) (1 + cos(pi u)) / 2
 * so f(w) = 1, f(T) = r, and f stays at r past T (T is not read under SRFRD_SCHED_CONSTANT).
 */
enum { SRFRD_SCHED_CONSTANT = 0, SRFRD_SCHED_LINEAR = 1, SRFRD_SCHED_COSINE = 2 };

typedef struct srfrd_optim_opts {
  double lr, beta1, beta2;         /* base rate, Adam betas */
  double weight_decay;             /* decoupled (AdamW): p *= 1 - lr_t * weight_decay ahead of the Adam update; >= 0 */
  double final_ratio;              /* r, in [0, 1] */
  int64_t warmup_steps;            /* w >= 0 */
  int64_t total_steps;             /* T >= w under a decaying schedule */
  int32_t schedule;                /* SRFRD_SCHED_* */
  int32_t reserved;                /* 0 */
} srfrd_optim_opts;

/* srfrd_step_begin under a schedule: t += 1, next dropout seed, and with lr_t of the NEW t
 *   state[4] = float(lr_t / (1 - b1^t)), state[5] = float(sqrt(1 - b2^t))       (srfrd_step_begin's words, lr_t for lr)
 *   state[3] = float(lr_t), state[7] = float(1 - lr_t * weight_decay)           (the factor torch.optim.AdamW multiplies by)
 * Every other word stays untouched.  With SRFRD_SCHED_CONSTANT, no warmup and no decay words 0, 2, 4 and 5 are bitwise
 * srfrd_step_begin's.  SRFRD_E_ARG before any launch: state or opts NULL, a negative or NaN weight_decay, a negative
 * warmup_steps, a decaying schedule with total_steps < warmup_steps, an unknown schedule, final_ratio outside [0, 1]. */
int srfrd_step_begin_sched(uint32_t* state, const srfrd_optim_opts* opts, void* stream);

/* Workgroups, and fp64 partial sums, of srfrd_grad_norm at most: `partial` holds this many doubles. */
#define SRFRD_GRAD_NORM_PARTIALS 1024
/* Floats of one workgroup's share of the vector at least (shares grow, in steps of four floats, once n exceeds
 * SRFRD_GRAD_NORM_PARTIALS of them). */
#define SRFRD_GRAD_NORM_SHARE 4096

/*
 * Global L2 norm of the flat gradient and torch.nn.utils.clip_grad_norm_'s coefficient, deterministic:
 *   out[0] = sqrt(sum_i grad[i]^2) * gscale      gscale = 1 / stats[2] (the count the Adam step divides by), 1 if stats == NULL
 *   out[1] = min(1, max_norm / (out[0] + 1e-6))  max_norm = +inf only measures (coefficient 1); a NaN norm gives a NaN
 *                                                coefficient, as torch's clamp does
 * Squares and sums are fp64 (the square of a float is exact in a double).  Workgroup g of ceil(n4 / share4) sums the
 * contiguous floats [4 g share4, 4 (g + 1) share4), n4 = n / 4, share4 = max(SRFRD_GRAD_NORM_SHARE / 4, ceil(n4 /
 * SRFRD_GRAD_NORM_PARTIALS)): the split depends on n alone, never on the device.  A second one-wave kernel behind the
 * same entry point adds the partials - lane l its sixteen in index order, then the 64 lane sums in lane order, then the
 * n % 4 tail elements in index order - so two calls on the same data give the same bits.
 * grad is 16-byte aligned; partial: SRFRD_GRAD_NORM_PARTIALS doubles of workspace; out: 2 floats.
 * SRFRD_E_ARG before any launch: grad, partial or out NULL, grad misaligned, n <= 0, max_norm <= 0 or NaN.
 */
int srfrd_grad_norm(const float* grad, int64_t n, const float* stats, double max_norm, double* partial, float* out,
                    void* stream);

/*
 * srfrd_adam_step with clipping and decoupled weight decay: per element
 *   gs = gscale * coef (one float multiply; coef = clip[1], srfrd_grad_norm's out - 1 if clip == NULL);  g = grad[i] * gs;
 *   m, v as srfrd_adam_step;  p = p * state[7] - step_size * m / (sqrt(v) / bc2_sqrt + eps)
 * `state` comes from srfrd_step_begin_sched (words 4, 5, 7).  With clip == NULL and state[7] == 1 the result is bitwise
 * srfrd_adam_step's.  Argument checks as srfrd_adam_step.
 */
int srfrd_adamw_step(float* param, float* grad, float* m, float* v, int64_t n, int64_t i0, int64_t i1,
                     int64_t n_zero, double beta1, double beta2, double eps,
                     const uint32_t* state, const float* stats, const float* clip, uint16_t* table_bf16, int64_t n_table,
                     void* stream);

/* srfrd_adam_pack_step with srfrd_adamw_step's arithmetic; the last block to finish makes srfrd_step_begin_sched's advance
 * under `opts` (which also carries lr and the betas).  Argument checks: srfrd_adam_pack_step's and
 * srfrd_step_begin_sched's, all before any launch. */
int srfrd_adamw_pack_step(const srfrd_layout* lay, float* param, float* grad, float* m, float* v, int64_t n,
                          int64_t n_table_pad, int64_t n_zero, const srfrd_optim_opts* opts, double eps,
                          uint32_t* state, const float* stats, const float* clip, float* packed, uint16_t* table_bf16,
                          void* stream);

/* bf16 shadow of an fp32 vector (round to nearest even; fp32 denormals are rounded, not flushed; NaN stays NaN):
 * out[i] = bf16(src[i]), i < n.  Builds / refreshes the item-table
 * shadow that lay->table_bf16 = 1 launches gather from (the fused optimizer keeps it current by itself). */
int srfrd_table_to_bf16(const float* src, int64_t n, uint16_t* out, void* stream);

/* loss = stats[0]/stats[2] + stats[1]/stats[2] -> loss_out[0] (reference trainer.py:36-38). */
/* The `l2_emb * ||p||_2` terms of reference trainer.py:39 (one Frobenius norm per parameter tensor) for the fused step.
 * srfrd_l2_norms: the n_seg parameter tensors are [seg_off[k], seg_off[k] + seg_len[k]) of `param` (device int64 arrays;
 *   segment 0 = the item table, the others lie at or above n_table_pad); partial: 240 + n_seg floats of workspace;
 *   l2buf[0] = l2_emb / ||table||, l2buf[1] = l2_emb * sum_k ||p_k|| (add it to the loss); dense_scale (n_dense floats,
 *   zero-initialised by the caller once): l2_emb / ||p|| of the tensor each dense element belongs to.
 * srfrd_l2_apply: grad[i] += stats[2] * (l2_emb / ||p||) * param[i] over [i0, i1) (stats[2] = the count the Adam step
 *   divides by; NULL: 1) - enqueue between the gradient exchange and the Adam step of that range. */
int srfrd_l2_norms(const float* param, const int64_t* seg_off, const int64_t* seg_len, int n_seg, int64_t n_table_pad,
                   double l2_emb, float* partial, float* l2buf, float* dense_scale, void* stream);
int srfrd_l2_apply(float* grad, const float* param, int64_t i0, int64_t i1, int64_t n_table_pad, const float* l2buf,
                   const float* dense_scale, const float* stats, void* stream);

int srfrd_loss_finalize(const float* stats, float* loss_out, void* stream);

/* Which build is running: returns the wave mask the HOST code of this library was compiled with (-DSRFRD_SKEW=<mask>, the
 * schedule-skew diagnostic build of srfrd_dev.h; 0 in the product) and, when out_dev is not NULL, launches one thread that
 * stores the mask the DEVICE code was compiled with into out_dev[0].  Two builds loaded into one process carry the same
 * symbol names: a handle whose host and device answers both name its own mask runs its own code objects
 * (tests/test_gpu_skew_bits.py).  A launch failure reads as a negative return (-(hipError_t)), never as a mask. */
int srfrd_skew_mask(uint32_t* out_dev, void* stream);

/* get_Labels (reference SRFR_model.py:546-570) and SRFRN.predict's user label (:244); labels int64 (B).
 * kind = SRFRD_SRFU_B / _F / _R, or SRFRD_SRFRN for the predict label. */
int srfrd_user_labels(int kind, const int64_t* fake_ids, int B, int L, int64_t* labels, void* stream);

/*
 * Id validation.  The reference's nn.Embedding raises IndexError for an id outside its table (SRFR_model.py:10-12, 402-404,
 * 590-591); the fused kernels instead CLAMP every id into range (item ids to [0, n_items], fake ids to [0, 2]) so that no
 * input can read or scatter out of bounds, and this launcher reports the violation: err_word[0] |= 1 if any of the (up to
 * three, each may be NULL) item-id arrays holds an id outside [0, n_items], |= 2 if any fake-id array holds one outside
 * [0, fake_hi].  Each array has n elements.  The host reads the word when it next synchronises (srfrd_amd: check_ids()).
 */
int srfrd_check_ids(const int64_t* item_a, const int64_t* item_b, const int64_t* item_c,
                    const int64_t* fake_a, const int64_t* fake_b, const int64_t* fake_c,
                    int64_t n, int64_t n_items, int64_t fake_hi, uint32_t* err_word, void* stream);

/*
 * predict (reference SRFR_model.py:144-152 and twins): logits[b][i] = <hidden[b, L-1, :], E[cand]> with
 * E = item row (SRFRN: item row || fake_embed[user_label[b]]).  cand is (n_cand) shared by all users
 * (cand_stride = 0) or (B, n_cand) per user (cand_stride = n_cand).  logits (B, n_cand).
 */
int srfrd_predict_logits(const srfrd_layout* lay, const void* item_table, const float* dense,
                         const float* hidden, int B, int L, const int64_t* cand, int n_cand, int64_t cand_stride,
                         const int64_t* user_label, float* logits, void* stream);

/*
 * Full-catalog ranking: top-k items of <hidden[b, L-1, :], E[i]> over i in [item_lo, item_hi) with the logits
 * never written to HBM.  Ties break to the lower item id (stable descending sort).  topk_idx int64 (B,k),
 * topk_val (B,k).  workspace: srfrd_topk_workspace_bytes().  exclude_pad != 0 skips item 0.
 * A returned score is fp32-grade, not one fixed rounding: a candidate list that overflows (more than 2048 scores at or above
 * the k-th largest chunk maximum: mass ties, or fewer chunks than k over more than 2048 rows) is re-ranked by the exhaustive
 * path, whose fp32 matrix-core sum and the bf16 stream's six-product sum can round the same (user, item) score to
 * neighbouring floats.  Within one call all scores come from one arithmetic, so the order law holds exactly; across calls
 * (another k, another item range) two items whose scores lie within that rounding of each other may change places.
 */
int64_t srfrd_topk_workspace_bytes(int B, int k, int64_t n_rows);
int srfrd_logits_topk(const srfrd_layout* lay, const void* item_table, const float* dense,
                      const float* hidden, int B, int L, int64_t item_lo, int64_t item_hi, int exclude_pad,
                      const int64_t* user_label, int k, int64_t* topk_idx, float* topk_val,
                      void* workspace, void* stream);

/*
 * Merge of per-shard top-k lists: the catalog's rows split into shards (one per GPU for the row-sharded table of BASELINE
 * configs[4], or just to bound the ranking workspace), each ranked by srfrd_logits_topk over its [item_lo, item_hi).
 * cand_idx int64 / cand_val (B, n_cand) hold the shards' lists side by side (n_cand = shards * k <= 4096; idx < 0 marks an
 * empty slot); topk_idx / topk_val (B, k) receive the k best in stable descending order (value desc, item id asc), exact
 * ties across shard boundaries included.  That is what ONE srfrd_logits_topk over the whole catalog returns, bit for bit,
 * when the shards and the whole catalog are scored by the same arithmetic (see srfrd_logits_topk: every list on the
 * threshold scheme, e.g. k = 10); otherwise the ids agree wherever two scores differ by more than their rounding, and the
 * values agree to that rounding.
 */
int srfrd_topk_merge(const int64_t* cand_idx, const float* cand_val, int B, int n_cand, int k,
                     int64_t* topk_idx, float* topk_val, void* stream);

/*
 * Full-catalog ranking with per-user exclusion sets (items a user already has; the `rated` set of a full-catalog evaluation).
 * Row b's set is excl_items[excl_ptr[b] .. excl_ptr[b + 1]) (CSR over the batch: excl_ptr int64 (B + 1), excl_items int32):
 * unsorted, duplicates, ids outside [item_lo, item_hi) and 0 are all accepted; a row may be empty.  max_row [host] bounds
 * every row's length (the launchers read at most that many ids of a row); max_row > SRFRD_EXCL_CAP -> SRFRD_E_UNSUPPORTED.
 * A pre-pass sorts and deduplicates each row into the exclusion workspace; the ranking passes mask the excluded
 * (user, item) scores inside every pass (chunk maxima, threshold, collection, the exhaustive path).
 * excl_ptr == NULL: no exclusion (srfrd_logits_topk_excl then launches exactly what srfrd_logits_topk does).
 *
 * srfrd_logits_topk_excl: srfrd_logits_topk over {i in [item_lo, item_hi) : i not in excl[b], !(exclude_pad && i == 0)};
 *   fewer than k such items -> trailing slots idx -1 / val -inf.  workspace: srfrd_topk_workspace_bytes(B, k, n_rows),
 *   excl_workspace: srfrd_excl_workspace_bytes(B, max_row, n_rows) (n_rows = item_hi - item_lo).
 * srfrd_target_rank: rank[b] = #{i in [item_lo, item_hi) : i != t_b, i not in excl[b], !(exclude_pad && i == 0),
 *   s(b, i) > s(b, t_b)} with targets t (int64 (B)); s(b, t_b) is the score the ranking pass's own tile arithmetic gives
 *   t_b's row, so a bit-identical duplicate of the target ties and is not counted; t_b is ranked even when it is in its own
 *   set.  Ranks over disjoint item ranges add up.  metric_acc (double[3], may be NULL): [0] += [rank < cut_k] /
 *   log2(rank + 2), [1] += [rank < cut_k], [2] += 1.  workspace: srfrd_excl_workspace_bytes(B, max_row, n_rows) bytes
 *   (max_row 0 without exclusion).
 */
#define SRFRD_EXCL_CAP 4096
int64_t srfrd_excl_workspace_bytes(int B, int max_row, int64_t n_rows);
int srfrd_logits_topk_excl(const srfrd_layout* lay, const void* item_table, const float* dense,
                           const float* hidden, int B, int L, int64_t item_lo, int64_t item_hi, int exclude_pad,
                           const int64_t* user_label, int k, const int64_t* excl_ptr, const int32_t* excl_items, int max_row,
                           int64_t* topk_idx, float* topk_val, void* workspace, void* excl_workspace, void* stream);
int srfrd_target_rank(const srfrd_layout* lay, const void* item_table, const float* dense, const float* hidden,
                      int B, int L, int64_t item_lo, int64_t item_hi, int exclude_pad, const int64_t* user_label,
                      const int64_t* targets, const int64_t* excl_ptr, const int32_t* excl_items, int max_row,
                      int cut_k, int32_t* rank, double* metric_acc, void* workspace, void* stream);

/* [host] the ranking's kernel plan, asked without a GPU: the launches srfrd_logits_topk(_excl) (op SRFRD_RANK_TOPK) or
 * srfrd_target_rank (SRFRD_RANK_TARGET, or SRFRD_RANK_TARGET_METRIC with metric_acc != NULL) make for (lay, B, k,
 * [item_lo, item_hi)), with an exclusion set when excl != 0, under `switches` (SRFRD_SW_* bits, as srfrd_encoder_plan) on a
 * device with n_cu CUs.  For launch i < max_launches, in launch order: its kernel's name as a kernel trace prints it,
 * without spaces ("srfrd::topk_max16_kernel<2,true,false>"; names + i * name_len, at most name_len bytes with the NUL)
 * and geom[3 i ..]: workgroups, threads per workgroup, dynamic LDS bytes (names / geom may be NULL).  Returns the number of
 * launches, SRFRD_E_UNSUPPORTED where the call refuses (it then launches nothing), or SRFRD_E_ARG. */
#define SRFRD_RANK_TOPK 0
#define SRFRD_RANK_TARGET 1
#define SRFRD_RANK_TARGET_METRIC 2
int srfrd_rank_plan(const srfrd_layout* lay, int op, int B, int k, int64_t item_lo, int64_t item_hi, int excl, int switches,
                    int n_cu, int max_launches, char* names, int name_len, int32_t* geom);

/* HR@10 / NDCG@10 inputs (reference utils.py:589-597): rank[b] = #{i >= 1 : logits[b][i] > logits[b][0]};
 * metric_acc[0] += [rank<10] / log2(rank+2), metric_acc[1] += [rank<10], metric_acc[2] += 1 (double[3]).
 * The compare is IEEE on the float32 values (a denormal is greater than 0; +0 and -0 tie).  NaN: a NaN target
 * (logits[b][0]) counts every other candidate, rank n_cand - 1, which is where the reference's argsort puts it - a model
 * that has diverged to NaN scores reads as a miss, not as rank 0; a NaN competitor of a finite target is not counted.
 * rank and metric_acc may each be NULL. */
int srfrd_eval_rank(const float* logits, int B, int n_cand, int32_t* rank, double* metric_acc, void* stream);

/*
 * Full-catalog softmax cross-entropy (no reference counterpart: the reference trains with one sampled negative per position,
 * trainer.py:36-38).  Tokens are the positions t of the (B, L) `targets` with targets[t] != 0; the candidates are the items
 * 1..n_items (item 0, the pad row, is excluded); s_tj = <hidden[t, :d_item], E[j]> with E = the fp32 item table
 * (n_items + 1, d_item) and hidden (B, L, d_out) - SRFRN's fake slice is not read (it adds one constant per row, which the
 * softmax does not see); loss_t = logsumexp_j s_tj - s_t,y.  Target ids are clamped into [0, n_items] as everywhere else.
 * The (tokens x items) logits are never written: the forward streams the table in item tiles against tiles of tokens on
 * the fp32 matrix cores, the backward recomputes them.  No float atomics: two identical calls give bitwise-identical results.
 * lay->table_bf16 or lay->D > SRFRD_MAX_D -> SRFRD_E_UNSUPPORTED.
 *
 * srfrd_xent_workspace_floats [host]: floats of `workspace` both calls need for (B, L) (0 for arguments they refuse).
 * srfrd_xent_fwd: token_loss (B, L) (0 where targets == 0), lse (B, L) (0 there too), stats[0..1] = {sum of the token losses,
 *   token count} (fp32; the count stays on the device: a mean needs no host synchronisation).
 * srfrd_xent_bwd: with the forward's lse and the upstream gradient of every token loss d_token_loss (B, L):
 *   d_hidden (B, L, d_out) = sum_j d_t (softmax_tj - [j == y_t]) E[j] in columns < d_item, zeros elsewhere and at ignored
 *   positions (fully overwritten); grad_table (n_items + 1, d_item) = (accumulate: +=) sum_t d_t (softmax_tj - [j == y_t])
 *   hidden[t, :d_item]; row 0 receives 0.
 */
int64_t srfrd_xent_workspace_floats(const srfrd_layout* lay, int B, int L);
int srfrd_xent_fwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets, int B, int L,
                   float* token_loss, float* lse, float* stats, float* workspace, int64_t ws_floats, void* stream);
int srfrd_xent_bwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                   const float* lse, const float* d_token_loss, int B, int L, float* d_hidden, float* grad_table,
                   int accumulate, float* workspace, int64_t ws_floats, void* stream);

/*
 * Sampled softmax cross-entropy with shared negatives (no reference counterpart either).  Tokens are the positions t of the
 * (B, L) `targets` with targets[t] != 0, as in srfrd_xent_*.  `negatives` (K) int64 is one set of sampled item ids shared by
 * every token: id 0 marks an unused slot, duplicates are allowed (each occurrence is its own candidate).  `log_q` (K) fp32
 * may be NULL.  s_t+ = <hidden[t, :d_item], E[y_t]>; slot j has s_tj = <hidden[t, :d_item], E[n_j]> - log_q[j] (nothing
 * subtracted without log_q); loss_t = logsumexp({s_t+} u {s_tj : n_j != 0, and n_j != y_t if remove_hits}) - s_t+, which is
 * 0 with a zero gradient when no slot takes part.  negatives = 1..n_items without log_q and with remove_hits is the full-
 * catalog loss.  SRFRN's fake slice is not read (one constant per row: the softmax does not see it).  Ids are clamped into
 * [0, n_items].  The (tokens x (1 + K)) logits are never written: the forward streams 64-slot chunks of gathered rows E[n_j]
 * against tiles of tokens on the fp32 matrix cores, the backward recomputes them.  No float atomics: two identical calls
 * give bitwise-identical results.  lay->table_bf16 or lay->D > SRFRD_MAX_D -> SRFRD_E_UNSUPPORTED; K <= 0 -> SRFRD_E_ARG.
 *
 * srfrd_sxent_workspace_floats [host]: floats of `workspace` both calls need for (B, L, K) (0 for arguments they refuse).
 * srfrd_sxent_fwd: token_loss (B, L) (0 where targets == 0), lse (B, L) (0 there too; the log of the sampled partition
 *   function, target term included), stats[0..1] = {sum of the token losses, token count} (fp32, on the device).
 * srfrd_sxent_bwd: with the forward's lse and the upstream gradient of every token loss d_token_loss (B, L):
 *   d_hidden (B, L, d_out) = sum_j d_t softmax_tj E[n_j] + d_t (softmax_t+ - 1) E[y_t] in columns < d_item, zeros elsewhere
 *   and at ignored positions (fully overwritten).  The table gradient is left unsummed, in the srfrd_table_reduce contract:
 *   table_contrib (K + B L, d_item) and contrib_keys (K + B L) int64, fully overwritten.  Row j < K is slot j's
 *   sum_t d_t softmax_tj hidden[t, :d_item] with key n_j; row K + t is d_t (softmax_t+ - 1) hidden[t, :d_item] with key
 *   y_t.  Unused slots and positions without a target have key 0 and a zero row.  A stable sort of the keys followed by
 *   srfrd_table_reduce into a zeroed (n_items + 1, d_item) gradient gives dE with every item's rows summed in a fixed order.
 */
int64_t srfrd_sxent_workspace_floats(const srfrd_layout* lay, int B, int L, int K);
int srfrd_sxent_fwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                    const int64_t* negatives, const float* log_q, int K, int remove_hits, int B, int L, float* token_loss,
                    float* lse, float* stats, float* workspace, int64_t ws_floats, void* stream);
int srfrd_sxent_bwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                    const int64_t* negatives, const float* log_q, int K, int remove_hits, const float* lse,
                    const float* d_token_loss, int B, int L, float* d_hidden, float* table_contrib, int64_t* contrib_keys,
                    float* workspace, int64_t ws_floats, void* stream);

/*
 * Losses with K negatives PER POSITION (the form the reference samples in, utils.py:27-46, with more than one of them):
 * sampled softmax with per-position negatives, and BCE with K negatives generalised to gBCE (gSASRec, Petrov & Macdonald,
 * RecSys 2023).  Tokens are the positions t of the (B, L) `targets` with targets[t] != 0.  `negatives` (B, L, K) int64: id 0
 * marks an unused slot, duplicates count once each, ids are clamped into [0, n_items].  s_t+ = <hidden[t, :d_item], E[y_t]>,
 * s_tk = <hidden[t, :d_item], E[n_tk]>; slot k takes part when n_tk != 0 and, with remove_hits, n_tk != y_t.
 *   SRFRD_TNEG_SOFTMAX  loss_t = logsumexp({s_t+} u {s_tk - log_q[t, k]}) - s_t+; log_q (B, L, K) fp32 or NULL.  A token
 *                       without a participating slot has loss 0 and a zero gradient, exactly.  SRFRN's fake slice is not
 *                       read (one constant per row: the softmax does not see it).
 *   SRFRD_TNEG_GBCE     loss_t = beta softplus(-s_t+) + sum_k softplus(s_tk), beta >= 0 finite (1: plain BCE with K
 *                       negatives; K = 1 too: the reference's loss, trainer.py:36-38, before its division by the count).
 *                       log_q must be NULL.  lay->kind == SRFRD_SRFRN -> SRFRD_E_UNSUPPORTED: its logits include the fake
 *                       slice, and BCE, unlike the softmax, is not invariant to that per-row term.
 * No row is shared between tokens: the logits are gathered rows against one hidden row on the vector ALU, a wave per
 * position, never written to memory; the backward recomputes them.  No float atomics: two identical calls give bitwise-
 * identical results.  lay->table_bf16 or lay->D > SRFRD_MAX_D -> SRFRD_E_UNSUPPORTED; a null pointer, K <= 0, B L (1 + K)
 * >= 2^31, an unknown objective, log_q with gbce, a negative or non-finite beta -> SRFRD_E_ARG.
 *
 * srfrd_tneg_workspace_floats [host]: floats of `workspace` the three calls need for (B, L, K) (0 for arguments they refuse).
 * srfrd_tneg_fwd: token_loss (B, L) (0 where targets == 0), lse (B, L) (softmax: the log of the sampled partition function,
 *   target term included; gbce and ignored positions: 0), stats[0..1] = {sum of the token losses, token count} (fp32, on the
 *   device: the contract of srfrd_sxent_fwd).
 * srfrd_tneg_bwd: with the forward's lse and the upstream gradient of every token loss d_token_loss (B, L): d_hidden
 *   (B, L, d_out) = g_t+ E[y_t] + sum_k g_tk E[n_tk] in columns < d_item, zeros elsewhere and at ignored positions (fully
 *   overwritten, by the kernel itself); softmax: g_t+ = d_t (softmax_t+ - 1), g_tk = d_t softmax_tk; gbce: g_t+ = -d_t beta
 *   sigmoid(-s_t+), g_tk = d_t sigmoid(s_tk).  The table gradient is left as a list of RANK-1 rows, never written out: row
 *   r = t (1 + K) + j is contrib_coef[r] * hidden[t, :d_item] with key contrib_keys[r]; j = 0 is the target (key y_t), j =
 *   1..K the negatives (key n_tk); slots that take no part and ignored positions have key 0 and coefficient 0.  contrib_coef
 *   (B, L, 1 + K) fp32 and contrib_keys (B, L, 1 + K) int64 are fully overwritten.
 * srfrd_table_reduce_rank1: the second half, as srfrd_table_reduce is for contribution rows: `sorted_keys` (n) the keys
 *   sorted ascending by a STABLE sort, order[i] the list row sorted position i came from; sums, per run of equal keys and in
 *   sorted order, contrib_coef[order[i]] * hidden[order[i] / rows_per_token, :d_item] into grad_table[key] (caller-zeroed
 *   (n_items + 1, d_item); rows without contributions are not touched; keys <= 0 are skipped, the segments that lie inside
 *   that run without being walked).  The sorted list is cut into segments of SRFRD_TNEG_SPLIT_ROWS rows summed by a wave
 *   each, so a popular item's long run costs no more than its share; a run that crosses segments has its per-segment
 *   partials added in segment order by a second launch.  The cut depends on the keys alone: bitwise reproducible.
 *   `workspace`: 2 ceil(n / SRFRD_TNEG_SPLIT_ROWS) d_item floats rounded up to 64 (srfrd_tneg_workspace_floats covers it
 *   for n = B L (1 + K)); n must be below 2^31.
 */
#define SRFRD_TNEG_SOFTMAX 0
#define SRFRD_TNEG_GBCE 1
#define SRFRD_TNEG_SPLIT_ROWS 256
int64_t srfrd_tneg_workspace_floats(const srfrd_layout* lay, int B, int L, int K);
int srfrd_tneg_fwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                   const int64_t* negatives, const float* log_q, int K, int objective, double beta, int remove_hits, int B,
                   int L, float* token_loss, float* lse, float* stats, float* workspace, int64_t ws_floats, void* stream);
int srfrd_tneg_bwd(const srfrd_layout* lay, const float* table, const float* hidden, const int64_t* targets,
                   const int64_t* negatives, const float* log_q, int K, int objective, double beta, int remove_hits,
                   const float* lse, const float* d_token_loss, int B, int L, float* d_hidden, float* contrib_coef,
                   int64_t* contrib_keys, float* workspace, int64_t ws_floats, void* stream);
int srfrd_table_reduce_rank1(const int64_t* sorted_keys, const int64_t* order, const float* contrib_coef,
                             const float* hidden, int d_out, int rows_per_token, int64_t n, int d_item, float* grad_table,
                             float* workspace, int64_t ws_floats, void* stream);

/*
 * srfrd_table_reduce_rank1 over a list that also holds FULL rows: the one table-gradient reduction of a train step whose
 * encoder backward leaves full contribution rows (table_contrib's input plane) and whose loss head leaves rank-1 rows
 * (srfrd_tneg_bwd).  Neither reduce adds to grad_table, so running both would need a dense add over the whole table.
 * The unsorted list has n entries: entry e < n_rows is rows[e, :d_item] (rows (n_rows, d_item) fp32), entry e >= n_rows the
 * rank-1 row contrib_coef[r] * hidden[r / rows_per_token, :d_item] with r = e - n_rows (so contrib_coef holds n - n_rows
 * floats and hidden (n - n_rows) / rows_per_token rows of d_out; both are only read).  sorted_keys / order: a STABLE
 * ascending sort of the concatenated keys.  Per run of equal keys the entries are summed in sorted order into
 * grad_table[key]: a full row enters as fmaf(1, row, acc), a rank-1 row as fmaf(coef, hidden, acc).  Keys <= 0 are skipped,
 * rows without contributions are not touched.  Segments, partials and merge are srfrd_table_reduce_rank1's (one kernel,
 * the row source a template parameter): bitwise reproducible, and with n_rows == 0 the bits of srfrd_table_reduce_rank1.
 * SRFRD_E_ARG before any launch: sorted_keys, order, grad_table or workspace NULL; rows NULL with n_rows > 0; contrib_coef
 * or hidden NULL with n > n_rows; n <= 0 or n > INT_MAX; n_rows < 0 or > n; rows_per_token < 1; d_item < 1 or >
 * SRFRD_MAX_D; d_out < d_item; ws_floats below srfrd_table_reduce_mixed_workspace_floats(n, d_item) [host] = 2 ceil(n /
 * SRFRD_TNEG_SPLIT_ROWS) d_item rounded up to 64 (0 for arguments the call refuses).
 */
int64_t srfrd_table_reduce_mixed_workspace_floats(int64_t n, int d_item);
int srfrd_table_reduce_mixed(const int64_t* sorted_keys, const int64_t* order, int64_t n, const float* rows, int64_t n_rows,
                             const float* contrib_coef, const float* hidden, int d_out, int rows_per_token, int d_item,
                             float* grad_table, float* workspace, int64_t ws_floats, void* stream);

/*
 * Shared negatives of one sampled-softmax train step, drawn on the device (FusedTrainer(loss="sampled_softmax") captures it
 * into the step graph).  Slot j < K: h1 = fmix32(base ^ j), h2 = fmix32(base ^ (j | 2^31)) with base = fmix32(state[2] +
 * SITE_NEG * 0x9E3779B9) (srfrd_rng.h; state[2] is the step seed word srfrd_step_begin / srfrd_adam_pack_step advance), then
 *   uniform (alias_prob == alias_idx == NULL): out_ids[j] = 1 + mulhi32(h1, n_items);
 *   alias (Walker / Vose table over buckets 0..n_items-1, alias_prob fp32 and alias_idx int32 (n_items)): b = mulhi32(h1,
 *     n_items), out_ids[j] = 1 + (u < alias_prob[b] ? b : alias_idx[b]) with u = (h2 >> 8) * 2^-24.
 * out_log_q[j] = item_log_q[out_ids[j]] (item_log_q fp32 (n_items + 1), e.g. log(K q)), or log(K / n_items) when item_log_q is
 * NULL (uniform only).  mulhi32(a, b) = (a * b) >> 32 in 64 bits.  K <= 0, n_items < 1, a NULL output, one of the two alias
 * arrays without the other, or an alias table without item_log_q -> SRFRD_E_ARG.
 */
int srfrd_shared_negatives(const uint32_t* state, int n_items, int K, const float* alias_prob, const int32_t* alias_idx,
                           const float* item_log_q, int64_t* out_ids, float* out_log_q, void* stream);

/*
 * K negatives PER POSITION for srfrd_tneg_fwd / _bwd, drawn on the device outside the row user's history (the reference's
 * random_neq, utils.py:14-19, used at :27-46, with K slots per position).  user_ptr / items are the CSR histories of
 * srfrd_sample_batch (user_ptr int64 (usernum + 2), items int32; time-ordered, duplicates allowed).  users (B) are the rows'
 * user ids, clamped into [0, usernum]; targets is (B, L) int64.  out_ids (B, L, K) int64, out_log_q (B, L, K) fp32 or NULL.
 *   - A position with targets == 0 gets id 0 and log_q 0 in all K slots.
 *   - A slot at a live position makes up to SRFRD_TNEG_TRIES draws and keeps the first candidate that is not among the
 *     user's training items: the WHOLE history, not only the last L (the position's own target is in it).  The kernel reads
 *     at most the first max_hist items of a history.
 *   - If all SRFRD_TNEG_TRIES draws clash, the slot is written as id 0 with log_q 0, which the loss treats as unused: a
 *     history item is never emitted (unlike the 256-try fallback of srfrd_sample_batch's one negative).
 *   - exclude_history == 0: the first draw is kept.
 *   - Slots of one position are independent: sampling is with replacement.
 * Stream (integer-exact, wrapping in uint32; fmix32 and SITE_TNEG = 0x4E470002 of srfrd_rng.h; mulhi32(a, b) = (a * b) >> 32
 * in 64 bits):
 *   s0 = fmix32(seed ^ batch_index * 0x9E3779B9)
 *   s1 = fmix32(s0 + SITE_TNEG * 0x9E3779B9 + (state ? state[2] : 0))     state: the optimizer's uint32 state words, state[2]
 *                                                                        the step seed: a captured graph draws afresh per replay
 *   s2 = fmix32(s1 + b),  e = fmix32(s2 ^ (t * K + k))
 *   try r: h1 = fmix32(e + 2r), h2 = fmix32(e + 2r + 1), bucket = mulhi32(h1, n_items)
 *   alias table given (as for srfrd_shared_negatives): u = (h2 >> 8) * 2^-24; if !(u < alias_prob[bucket]) bucket =
 *     clamp(alias_idx[bucket], 0, n_items - 1)
 *   id = bucket + 1
 * out_log_q[b, t, k] = (item_log_q ? item_log_q[id] : (float)log((double)K / n_items)) - (user_log_keep ? user_log_keep[u] : 0),
 * one fp32 subtraction.  item_log_q fp32 (n_items + 1) is log(K q); user_log_keep fp32 (usernum + 1) is log(1 - the sum of q
 * over the distinct items of u's history), the renormalisation that rejection imposes on q.
 * One 256-thread workgroup per sequence; with exclusion the user's items go into an open-addressing set in dynamic LDS
 * (4 bytes x the power of two >= 2 max(max_hist, 32)); plain stores only, every output element written exactly once by the
 * kernel, two identical calls give identical bits.
 * Refused before any launch: a NULL user_ptr, items, users, targets or out_ids, B, L, K, usernum or n_items <= 0, B L (1 + K)
 * >= 2^31, one of the two alias arrays without the other, an alias table without item_log_q, max_hist < 0 -> SRFRD_E_ARG;
 * exclude_history with max_hist > SRFRD_TNEG_MAX_HIST -> SRFRD_E_UNSUPPORTED.
 */
#define SRFRD_TNEG_TRIES 32
#define SRFRD_TNEG_MAX_HIST 16384
int srfrd_token_negatives(const int64_t* user_ptr, const int32_t* items, int usernum, int n_items, int max_hist,
                          const int64_t* users, const int64_t* targets, int B, int L, int K,
                          uint32_t seed, uint32_t batch_index, const uint32_t* state,
                          const float* alias_prob, const int32_t* alias_idx, const float* item_log_q,
                          const float* user_log_keep, int exclude_history,
                          int64_t* out_ids, float* out_log_q, void* stream);

/*
 * Device-side batch sampler with the layout and semantics of reference utils.py:21-57 (sample_function_fr /
 * WarpSampler_fr): per sampled user (uniform among users with > 1 interaction) the most recent `L` training items
 * left-padded with 0, pos[t] = the next item, neg[t] = a uniform item outside the user's history wherever pos[t] != 0,
 * rsq / prs the fake(1)/real(2) ids, nrs = 1 where set.  Histories are CSR over user ids 0..usernum:
 * user_ptr int64 (usernum + 2), items / reviews int32.  out_packed int64 (6, B, L) = [seq, rsq, pos, prs, neg, nrs].
 * Randomness: counter hash of (seed, batch_index, row, position, try) - reproducible, unlike the reference's
 * unseeded worker processes (utils.py:79).
 * A row draws at most 4096 users: when none of them has more than one interaction the row comes out all-pad (0 in all six
 * planes) and out_user names the last user drawn.  A negative draws at most 256 candidates: when every one is among the
 * user's items (a user who holds the whole catalog) the negative is the last candidate, a history item.
 */
int srfrd_sample_batch(const int64_t* user_ptr, const int32_t* items, const int32_t* reviews, int usernum, int itemnum,
                       int B, int L, uint32_t seed, uint32_t batch_index, int64_t* out_user, int64_t* out_packed,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRFRD_HIP_H */
