// Fused SRFRD encoder FORWARD for MI355X (gfx950).
//
// One persistent workgroup walks sequences b = blockIdx.x, blockIdx.x + gridDim.x, ...; the whole per-sequence
// working set (embedded inputs, LN outputs, Q/K/V, the L x L scores, FFN hidden) stays in LDS between phases, so HBM
// sees only ids, the gathered embedding rows, the outputs and (training) the per-block checkpoints.  Reference
// arithmetic being reproduced: SURVEY.md 3.4 / reference SRFR_model.py:92-142 (SRFR), :192-239 (SRFRN), :473-530
// (SRFU_*), :621-666 (SASRec); torch multi_head_attention_forward explicit path (q from LN(x), k = v from x,
// q * sqrt(1/d_h), additive causal -inf mask, softmax, dropout on P, P v, out_proj); residuals on the LayerNormed
// tensors; eps = 1e-8.
#include "srfrd_enc_common.h"

#include "srfrd_encoder_fwd_kernel.inc"

namespace srfrd {
// ================================================================================================
// weight packing: canonical (N, K) row-major weights -> MFMA B-fragment order, both product forms
// ================================================================================================
__global__ void __launch_bounds__(256) pack_weights_kernel(const srfrd_layout ly, const float* __restrict__ dense,
                                                          float* __restrict__ packed, uint32_t* state, double lr, double b1,
                                                          double b2) {
  // the last launch of a fused train step also advances the optimizer state for the NEXT step (saves a launch)
  if (state != nullptr && blockIdx.x == 0 && threadIdx.x == 0) step_advance(state, lr, b1, b2);
  const int mf = blockIdx.x, mat = mf >> 1, form = mf & 1;
  const int nb6 = ly.n_blocks * 6;
  const float* W;
  int N, K;
  if (mat < nb6) {
    const srfrd_block_off o = ly.blk[mat / 6];
    const int m = mat % 6, D = ly.D;
    W = dense + (m < 3 ? o.in_w + (int64_t)m * D * D : m == 3 ? o.out_w : m == 4 ? o.c1_w : o.c2_w);
    N = K = D;
  } else {
    if (ly.off_lc_w < 0) return;
    W = dense + ly.off_lc_w;
    N = ly.d_item;
    K = ly.D;
  }
  for (int idx = threadIdx.x; idx < kPackFloats; idx += blockDim.x) {
    const int s = idx & 3, lane = (idx >> 2) & 63, kc = (idx >> 8) & 3, nt = idx >> 10;
    const int k = kc * 16 + 4 * s + (lane >> 4), n = nt * 16 + (lane & 15);
    float v;
    if (form == 0) v = (n < N && k < K) ? W[n * K + k] : 0.f;      // B(k, n) = W[n][k]   (x W^T)
    else v = (k < N && n < K) ? W[k * K + n] : 0.f;                // B(k, n) = W[k][n]   (dy W)
    packed[(int64_t)mf * kPackFloats + idx] = v;
  }
}

}  // namespace srfrd

using namespace srfrd;

// floats of the caller's scratch per workgroup of a global-scratch build
static int64_t scratch_stride(int64_t lds_floats) { return (lds_floats + 2 * kSlack + 63) & ~63ll; }

extern "C" int64_t srfrd_aux_floats(const srfrd_layout* lay, int B, int L) {
  if (!lay || B <= 0 || L <= 0) return SRFRD_E_ARG;
  const Geom g = make_geom(L, lay->D);
  return (int64_t)lay->n_blocks * B * aux_seq_floats(L, g.LP, lay->D, lay->n_heads);
}

extern "C" int srfrd_scratch_floats(const srfrd_layout* lay, int B, int L, int64_t* fwd_floats, int64_t* bwd_floats) {
  if (!lay || B <= 0 || L <= 0) return SRFRD_E_ARG;
  const Geom g = make_geom(L, lay->D);
  const int64_t f = fwd_lds_floats(g, lay->n_blocks), bw = bwd_lds_floats(g, lay->n_blocks);
  int gf = num_cu();
  if (gf > B) gf = B;
  if (fwd_floats) *fwd_floats = f * 4 <= kLdsLimit ? 0 : scratch_stride(f) * gf;
  if (bwd_floats) *bwd_floats = bw * 4 <= kLdsLimit ? 0 : scratch_stride(bw) * bwd_grid(*lay, B, L, num_cu());
  return 0;
}

extern "C" int srfrd_lds_bytes(const srfrd_layout* lay, int L, int64_t* fwd_bytes, int64_t* bwd_bytes) {
  if (!lay || L <= 0) return SRFRD_E_ARG;
  const Geom g = make_geom(L, lay->D);
  const int64_t f = fwd_lds_floats(g, lay->n_blocks) * 4, bw = bwd_lds_floats(g, lay->n_blocks) * 4;
  if (fwd_bytes) *fwd_bytes = f <= kLdsLimit ? f : 0;
  if (bwd_bytes) *bwd_bytes = bw <= kLdsLimit ? bw : 0;
  return 0;
}

extern "C" int64_t srfrd_packed_floats(const srfrd_layout* lay) {
  if (!lay) return 0;
  return (int64_t)(lay->n_blocks * 6 + 1) * 2 * kPackFloats;
}

extern "C" int srfrd_pack_weights(const srfrd_layout* lay, const float* dense, float* packed, uint32_t* state, double lr,
                                  double beta1, double beta2, void* stream) {
  if (!lay || !dense || !packed) return SRFRD_E_ARG;
  if (lay->D > SRFRD_MAX_D) return SRFRD_E_UNSUPPORTED;
  hipLaunchKernelGGL(pack_weights_kernel, dim3((lay->n_blocks * 6 + 1) * 2), dim3(256), 0, (hipStream_t)stream, *lay, dense,
                     packed, state, lr, beta1, beta2);
  return (int)hipGetLastError();
}

extern "C" int srfrd_debug_shape(const srfrd_layout* lay, int L, int64_t* slot_floats, int32_t* n_slots) {
  if (!lay || L <= 0) return SRFRD_E_ARG;
  if (slot_floats) *slot_floats = (int64_t)L * (L > lay->D ? L : lay->D);
  if (n_slots) *n_slots = 1 + 8 * lay->n_blocks;
  return 0;
}

// ================================================================================================
// kernel plan (srfrd_enc_plan.h): the one place that chooses an instantiation
// ================================================================================================
namespace srfrd {

int bwd_grid(const srfrd_layout& lay, int B, int L, int n_cu) {
  // The reference's default geometry (seq_len 50, hidden 50: BASELINE configs[1] / [2]) runs the slot-placed or ragged
  // backward with six [52][54] slots = 76 KB of LDS: TWO workgroups per CU, where the first-generation kernel's ten
  // matrices (150 KB) allow one.  A function of the shape only (never of the switches: callers size `grad_slabs` with it).
  const int wgs = n_cu * (L == 50 && kind_variant(lay) >= 0 ? 2 : 1);
  return B < wgs ? B : wgs;
}

static KernelPlan kernel(Family fam, int form, int variant, bool flag, int grid, int threads, int64_t lds, int64_t stride = 0) {
  return KernelPlan{0, fam, form, variant, flag, grid, threads, lds, stride};
}
static KernelPlan unsupported() { return KernelPlan{SRFRD_E_UNSUPPORTED, 0, 0, -1, false, 0, 0, 0, 0}; }
static bool fits(int64_t floats) { return floats * 4 <= kLdsLimit; }

EncPlan encoder_plan(const srfrd_layout& lay, int B, int L, int mode, int sw, int n_cu, int64_t scratch_floats) {
  const Geom g = make_geom(L, lay.D);
  const int nb = lay.n_blocks, kv = kind_variant(lay);
  const bool taps = mode & SRFRD_PLAN_TAPS;
  const bool generic = sw & SRFRD_SW_GENERIC;
  // the hidden-50, one-head instantiations (several attention heads: the generic instantiation only)
  const bool spec = !generic && lay.D == 50 && lay.n_heads == 1;
  const int kFwdTrain = SRFRD_PLAN_POS | SRFRD_PLAN_NEG | SRFRD_PLAN_CKPT | SRFRD_PLAN_LOSS | SRFRD_PLAN_DROPOUT;
  const int kBwdTrain = SRFRD_PLAN_POS | SRFRD_PLAN_NEG | SRFRD_PLAN_FUSED_BCE | SRFRD_PLAN_DROPOUT;
  const bool fwd_train = (mode & kFwdTrain) == kFwdTrain && !taps, bwd_train = (mode & kBwdTrain) == kBwdTrain && !taps;
  const bool plain = (mode & kFwdTrain) == 0;          // eval-mode hidden states only
  // The ragged seq_len-50 pair exchanges checkpoints that hold only the rows of the computed tiles: the forward and the
  // backward take it from this ONE decision.  Debug taps want every row of every intermediate: the full kernels.
  const bool ragged = L == 50 && kv >= 0 && !taps && !(sw & (SRFRD_SW_NO_RAGGED | SRFRD_SW_GENERIC | SRFRD_SW_NO_SLOTS50 | SRFRD_SW_ROWS_ALWAYS)) &&
                      fits(fwd_lds_floats(g, nb)) && fits(bwd_ragged_lds_floats(nb));
  EncPlan p;

  // ---- forward ----
  const int64_t fl = fwd_lds_floats(g, nb);
  const int fgrid_cu = n_cu < B ? n_cu : B;
  // the row-owner kernel (K / V resident in LDS): every long sequence it covers.  (Measured against the first-generation
  // kernel where both fit: 185 vs 170 us per 512-sequence training forward at seq_len 100, 117 vs 59 us at seq_len 50 - with
  // 7 or 4 row tiles it runs one or two waves per SIMD and their dependent chains are exposed; SRFRD_ROWS_ALWAYS selects it
  // anyway, for tests.)
  if ((!fits(fl) || (sw & SRFRD_SW_ROWS_ALWAYS)) && !taps && kv >= 0 && !(sw & (SRFRD_SW_NO_ROWS | SRFRD_SW_GENERIC)) &&
      L <= 16 * kRowMaxTiles && fits(rows_lds_floats(L, 50, nb))) {
    p.fwd = kernel(kFwdRows, kGeneric, kv, !plain, fgrid_cu, kRowWaves * 64, rows_lds_floats(L, 50, nb) * 4);
  } else if (!fits(fl)) {                 // long sequence: working set in the caller's global scratch
    const int64_t stride = scratch_stride(fl);
    p.fwd = scratch_floats < stride * fgrid_cu ? unsupported()
                                               : kernel(kFwdLong, kGeneric, -1, false, fgrid_cu, 256, (kLdsLimit / 4 - 64) * 4ll, stride);
  } else {
    const int per_cu = (int)(kLdsLimit / (fl * 4)) > 2 ? 2 : (int)(kLdsLimit / (fl * 4));
    int grid = n_cu * (per_cu < 1 ? 1 : per_cu);
    if (grid > B) grid = B;
    // 8 waves per workgroup measured fastest for the forward (95 vs 118 us at C2 with 4 waves)
    if (ragged) p.fwd = kernel(kFwdRagged, kGeneric, kv, fwd_train, grid, 512, fl * 4);
    else if (spec && L == 50) p.fwd = kernel(kFwdFirst, kL50, kv, kv >= 0 && fwd_train, grid, 512, fl * 4);
    // BASELINE configs[3] geometry (seq_len 100): still LDS-resident in the forward, one workgroup per CU.  The training
    // instantiation runs 16 waves (7 x 4 tiles per weight GEMM: two rounds instead of three and a half; 0.468 -> 0.462 ms
    // per C4 step - the 128-register budget of a 1024-thread workgroup takes back most of what the extra waves give)
    else if (spec && L == 100 && lay.kind == SRFRD_SASREC) p.fwd = kernel(kFwdFirst, kL100, 0, fwd_train, grid, fwd_train ? 1024 : 512, fl * 4);
    else if (spec && g.LP == 64) p.fwd = kernel(kFwdFirst, kLP64, -1, false, grid, 512, fl * 4);
    else if (spec && g.LP == 32) p.fwd = kernel(kFwdFirst, kLP32, -1, false, grid, 512, fl * 4);
    else p.fwd = kernel(kFwdFirst, kGeneric, -1, false, grid, 512, fl * 4);
  }

  // ---- backward ----
  const int64_t bl = bwd_lds_floats(g, nb);
  const int grid = bwd_grid(lay, B, L, n_cu);
  const bool rmw = B > grid;              // some workgroup takes a second sequence: its slab entries are read-modify-written
  const int64_t stride = scratch_stride(bl);
  const bool slots = (L == 50 || L == 100) && kv >= 0 && !taps && fits(slots_lds_floats(L, 50, nb));
  if (ragged) {
    p.bwd = kernel(kBwdRagged, kGeneric, kv, rmw, grid, 512, bwd_ragged_lds_floats(nb) * 4);
  } else if (slots && L == 50 && !(sw & (SRFRD_SW_NO_SLOTS50 | SRFRD_SW_GENERIC))) {
    // seq_len 50 (fused training step or autograd backward): the slot-placed kernel, two workgroups per CU.  (The switches
    // select the first-generation kernel on the same grid - one sequence per workgroup, half of them resident at a time.)
    p.bwd = kernel(kBwdSlots, kL50, kv, rmw, grid, kSlotWaves * 64, slots_lds_floats(L, 50, nb) * 4);
  } else if (!fits(bl) && !taps && kv >= 0 && !(sw & (SRFRD_SW_NO_SLOTS | SRFRD_SW_GENERIC)) && slots) {
    // a long sequence (fused training step or autograd backward): the slot-placed, query-chunked LDS-resident kernel where
    // one is built, the row-chunked one for the other lengths up to 208
    p.bwd = kernel(kBwdSlots, L == 50 ? kL50 : kL100, kv, rmw, grid, kSlotWaves * 64, slots_lds_floats(L, 50, nb) * 4);
  } else if (!fits(bl) && !taps && kv >= 0 && !(sw & (SRFRD_SW_NO_SLOTS | SRFRD_SW_GENERIC)) && scratch_floats >= stride * grid &&
             L >= 17 && L <= 208 && fits(chunks_lds_floats(L, 50, nb)) && stride >= chunks_scratch_floats(L, 50)) {
    p.bwd = kernel(kBwdChunks, kGeneric, kv, rmw, grid, kCkWaves * 64, chunks_lds_floats(L, 50, nb) * 4, stride);
  } else if (!fits(bl)) {                 // long sequence: working set in the caller's global scratch
    const bool c4 = spec && kv == 0 && L == 100 && bwd_train;
    p.bwd = scratch_floats < stride * grid ? unsupported()
                                           : kernel(kBwdLong, c4 ? kL100 : kGeneric, c4 ? 0 : -1, c4, grid, 512, (kLdsLimit / 4 - 64) * 4ll, stride);
  } else if (spec && L == 50) {
    p.bwd = kernel(kBwdFirst, kL50, kv, kv >= 0 && bwd_train, grid, 512, bl * 4);
  } else {
    p.bwd = kernel(kBwdFirst, spec && g.LP == 64 ? kLP64 : spec && g.LP == 32 ? kLP32 : kGeneric, -1, false, grid, 512, bl * 4);
  }

  // ---- train: forward and backward in one launch ----
  // Wherever the ragged pair serves a call that carries everything a fused train step computes (targets, checkpoints, loss
  // partials and the fused BCE gradient; dropout or not): the backward's grid, schedule and slab accumulation, so the two
  // launches and the one compute the same bits.
  const int kTrain = SRFRD_PLAN_POS | SRFRD_PLAN_NEG | SRFRD_PLAN_CKPT | SRFRD_PLAN_LOSS | SRFRD_PLAN_FUSED_BCE;
  p.train = ragged && (mode & kTrain) == kTrain && fits(train_ragged_lds_floats(nb))
                ? kernel(kTrainRagged, kGeneric, kv, rmw, grid, 512, train_ragged_lds_floats(nb) * 4)
                : unsupported();
  return p;
}

// template arguments of the first-generation kernels (all seven: a trace prints the defaults too)
static void first_targs(const KernelPlan& k, int t[7]) {
  const int gen[7] = {0, 0, 0, 0, -1, 0, 0};
  for (int i = 0; i < 7; ++i) t[i] = gen[i];
  if (k.form == kGeneric) return;
  t[0] = 50; t[2] = 8;
  t[1] = k.form == kLP32 ? 32 : k.form == kL100 ? 112 : 64;
  if (k.form == kL50 || k.form == kL100) {
    t[3] = k.form == kL50 ? 50 : 100;
    if (k.variant >= 0) { t[4] = kKindVariants[k.variant].K; t[5] = k.flag; t[6] = kKindVariants[k.variant].DI; }
    if (k.form == kL100 && k.family == kFwdFirst && k.flag) t[2] = 16;
  }
}

void plan_name(const KernelPlan& k, char* buf, int len) {
  if (len <= 0) return;
  buf[0] = 0;
  if (k.rc) return;
  const KindVariant v = kKindVariants[k.variant < 0 ? 3 : k.variant];
  const char* tf = k.flag ? "true" : "false";
  int t[7];
  switch (k.family) {
    case kFwdFirst: case kBwdFirst: case kFwdLong: case kBwdLong:
      first_targs(k, t);
      snprintf(buf, len, "%s::encoder_%s_kernel<%d,%d,%d,%d,%d,%d,%d>", k.family == kFwdLong || k.family == kBwdLong ? "srfrd_long" : "srfrd",
               k.family == kFwdFirst || k.family == kFwdLong ? "fwd" : "bwd", t[0], t[1], t[2], t[3], t[4], t[5], t[6]);
      return;
    case kFwdRows: snprintf(buf, len, "srfrd::encoder_fwd_rows_kernel<50,%d,%d,%d>", v.K, v.DI, (int)k.flag); return;
    case kFwdRagged: snprintf(buf, len, "srfrd::encoder_fwd_ragged_kernel<%d,%d,%d>", v.K, (int)k.flag, v.DI); return;
    case kBwdRagged: snprintf(buf, len, "srfrd::encoder_bwd_ragged_kernel<%d,%d,%s>", v.K, v.DI, tf); return;
    case kBwdSlots: snprintf(buf, len, "srfrd::encoder_bwd_slots_kernel<50,%d,%d,%d,%s>", k.form == kL50 ? 50 : 100, v.K, v.DI, tf); return;
    case kBwdChunks: snprintf(buf, len, "srfrd::encoder_bwd_chunks_kernel<50,%d,%d,%s>", v.K, v.DI, tf); return;
    case kTrainRagged: snprintf(buf, len, "srfrd::encoder_train_ragged_kernel<%d,%d,%s>", v.K, v.DI, tf); return;
  }
}

int launch_fwd_first(const KernelPlan& k, const EncArgs& a, void* stream) {
  switch (k.form) {
    case kL50:
      if (k.variant < 0) return launch_enc(encoder_fwd_kernel<50, 64, 8, 50>, k, stream, a);
      return with_variant_flag(k, [&](auto K, auto DI, auto t) { return launch_enc(encoder_fwd_kernel<50, 64, 8, 50, K, t, DI>, k, stream, a); });
    case kL100:
      return k.flag ? launch_enc(encoder_fwd_kernel<50, 112, 16, 100, SRFRD_SASREC, 1, 50>, k, stream, a)
                    : launch_enc(encoder_fwd_kernel<50, 112, 8, 100, SRFRD_SASREC, 0, 50>, k, stream, a);
    case kLP64: return launch_enc(encoder_fwd_kernel<50, 64, 8>, k, stream, a);
    case kLP32: return launch_enc(encoder_fwd_kernel<50, 32, 8>, k, stream, a);
    default: return launch_enc(encoder_fwd_kernel<0, 0, 0>, k, stream, a);
  }
}

}  // namespace srfrd

extern "C" int srfrd_encoder_plan(const srfrd_layout* lay, int B, int L, int mode, int switches, int n_cu, int64_t scratch_floats,
                                  char* fwd_name, char* bwd_name, int name_len, int32_t* grids) {
  if (!lay || B <= 0 || L <= 0 || n_cu <= 0 || scratch_floats < 0 || !grids) return SRFRD_E_ARG;
  EncPlan p = {unsupported(), unsupported(), unsupported()};
  if (layout_supported(*lay)) p = encoder_plan(*lay, B, L, mode, switches, n_cu, scratch_floats);
  if (fwd_name) plan_name(p.fwd, fwd_name, name_len);
  if (bwd_name) plan_name(p.bwd, bwd_name, name_len);
  grids[0] = p.fwd.rc ? p.fwd.rc : p.fwd.grid;
  grids[1] = p.bwd.rc ? p.bwd.rc : p.bwd.grid;
  return 0;
}

extern "C" int srfrd_encoder_plan_train(const srfrd_layout* lay, int B, int L, int mode, int switches, int n_cu, int64_t scratch_floats,
                                        char* name, int name_len, int32_t* grid) {
  if (!lay || B <= 0 || L <= 0 || n_cu <= 0 || scratch_floats < 0 || !grid) return SRFRD_E_ARG;
  const KernelPlan k = layout_supported(*lay) ? encoder_plan(*lay, B, L, mode, switches, n_cu, scratch_floats).train : unsupported();
  if (name) plan_name(k, name, name_len);
  *grid = k.rc ? k.rc : k.grid;
  return 0;
}

// ---- from a call to a launch: every launching entry point of the encoder goes through enc_run ----
namespace srfrd {
// the refusals every pass shares, and the kernels' view of the layout, the inputs and the dropout
static int fill_args(EncArgs& a, const EncCall& c) {
  const srfrd_layout* lay = c.lay;
  if (!lay || !c.item_table || !c.dense || !c.packed || !c.input_ids || c.B <= 0 || c.L <= 0) return SRFRD_E_ARG;
  if (!layout_supported(*lay)) return SRFRD_E_UNSUPPORTED;
  if (c.L > lay->max_len) return SRFRD_E_ARG;
  if (c.dropout_p < 0.0 || c.dropout_p >= 1.0) return SRFRD_E_ARG;
  if (lay->kind == SRFRD_SRFRN && ((c.pos_ids && !c.pos_fake) || (c.neg_ids && !c.neg_fake))) return SRFRD_E_ARG;
  Dims& d = a.dm;
  d.kind = lay->kind; d.d_item = lay->d_item; d.d_fake = lay->d_fake; d.D = lay->D; d.d_out = lay->d_out;
  d.n_labels = lay->n_labels; d.n_blocks = lay->n_blocks; d.n_items = lay->n_items; d.n_heads = lay->n_heads;
  d.off_pos = (int)lay->off_pos; d.off_side = (int)lay->off_side;
  d.blk0 = lay->n_blocks > 0 ? (int)lay->blk[0].ln1_w : 0;
  d.blk_stride = blk_stride_of(lay->D);
  for (int i = 0; i < lay->n_blocks; ++i) {        // the kernels recompute block offsets arithmetically: check the table agrees
    const BlkOff o = blk_off(d.blk0 + i * d.blk_stride, lay->D);
    const srfrd_block_off& t = lay->blk[i];
    if (t.ln1_w != o.ln1_w || t.ln1_b != o.ln1_b || t.in_w != o.in_w || t.in_b != o.in_b || t.out_w != o.out_w ||
        t.out_b != o.out_b || t.ln2_w != o.ln2_w || t.ln2_b != o.ln2_b || t.c1_w != o.c1_w || t.c1_b != o.c1_b ||
        t.c2_w != o.c2_w || t.c2_b != o.c2_b)
      return SRFRD_E_ARG;
  }
  d.off_lc_w = (int)lay->off_lc_w; d.off_lc_b = (int)lay->off_lc_b; d.off_ll_w = (int)lay->off_ll_w; d.off_ll_b = (int)lay->off_ll_b;
  d.n_dense = (int)lay->n_dense;
  d.flags = lay->flags;
  a.table = lay->table_bf16 ? nullptr : (const float*)c.item_table;
  a.table16 = lay->table_bf16 ? (const uint16_t*)c.item_table : nullptr;
  a.dense = c.dense; a.packed = c.packed;
  a.in_ids = c.input_ids; a.fk_ids = c.fake_ids; a.pos_ids = c.pos_ids; a.pos_fk = c.pos_fake; a.neg_ids = c.neg_ids; a.neg_fk = c.neg_fake;
  a.B = c.B; a.L = c.L; a.seed = c.seed; a.seed_dev = c.seed_dev;
  a.drop_on = c.dropout_p > 0.0;
  double thr = c.dropout_p * 4294967296.0;
  a.drop_thr = thr >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)thr;
  a.drop_scale = (float)(1.0 / (1.0 - c.dropout_p));
  a.seq0 = c.seq_index0;
  a.qscale = (float)sqrt(1.0 / (double)(lay->D / lay->n_heads));
  return 0;
}

// SRFRD_PLAN_* bits of a call: what it carries, as the plan's `mode` wants it
static int plan_mode(const EncCall& c, Pass pass) {
  int mode = (c.pos_ids ? SRFRD_PLAN_POS : 0) | (c.neg_ids ? SRFRD_PLAN_NEG : 0) | (c.dropout_p > 0.0 ? SRFRD_PLAN_DROPOUT : 0);
  if (pass != kBackward) mode |= (c.save_x || pass == kTrain ? SRFRD_PLAN_CKPT : 0) | (c.loss_part ? SRFRD_PLAN_LOSS : 0);
  if (pass != kForward) mode |= c.fused_bce && !c.d_hidden ? SRFRD_PLAN_FUSED_BCE : 0;
#ifndef SRFRD_STAMPS
  if (pass != kTrain && c.dbg) mode |= SRFRD_PLAN_TAPS;            // (diagnostic build: `dbg` receives the phase stamps, not taps)
#endif
  return mode;
}

int enc_run(const EncCall& c, Pass pass) {
  const bool fwd = pass != kBackward, bwd = pass != kForward;      // the train pass is both
  const int sw = read_switches();
  EncArgs a = {};
  a.sched = c.sched_mode != 0 ? c.sched : nullptr;
  a.sched_mode = a.sched ? c.sched_mode : 0;
  a.rank_G = c.rank_G; a.ragged_off = (sw & SRFRD_SW_RAGGED_FULL_ROWS) != 0;
  if (const int rc = fill_args(a, c)) return rc;
  // outputs and checkpoints
  if (fwd) {
    if (!c.hidden || (c.pos_ids && !c.pos_logits) || (c.neg_ids && !c.neg_logits)) return SRFRD_E_ARG;
    if (c.loss_part && !(c.pos_ids && c.neg_ids)) return SRFRD_E_ARG;
    if ((c.save_x != nullptr) != (c.save_h1 != nullptr) || (c.save_x != nullptr) != (c.save_aux != nullptr)) return SRFRD_E_ARG;
  }
  if (bwd) {
    if (!c.hidden || !c.save_x || !c.save_h1 || !c.save_aux || !c.grad_table || !c.grad_slabs) return SRFRD_E_ARG;
    if (c.fused_bce && !(c.pos_ids && c.neg_ids && c.pos_logits && c.neg_logits)) return SRFRD_E_ARG;
  }
  const EncPlan p = encoder_plan(*c.lay, c.B, c.L, plan_mode(c, pass), sw, num_cu(), c.scratch ? c.scratch_floats : 0);
  const KernelPlan& k = pass == kForward ? p.fwd : pass == kBackward ? p.bwd : p.train;
  if (k.rc) return k.rc;
  if (c.demand_scratch && (!c.scratch || c.scratch_floats < srfrd_train_scratch_floats(c.lay, c.B, c.L))) return SRFRD_E_ARG;
  if (fwd) {
    a.hidden = c.hidden; a.pos_logits = c.pos_logits; a.neg_logits = c.neg_logits; a.last_only = c.last_only;
    a.save_x = c.save_x; a.save_h1 = c.save_h1; a.save_aux = c.save_aux; a.loss_part = c.loss_part;
  }
  if (bwd) {                                   // (the train pass: what its forward half has just written)
    a.c_hidden = c.hidden; a.c_pl = c.pos_logits; a.c_nl = c.neg_logits; a.c_save_x = c.save_x; a.c_save_h1 = c.save_h1; a.c_save_aux = c.save_aux;
    a.grad_table = c.grad_table; a.grad_slabs = c.grad_slabs; a.contrib = c.table_contrib;
    a.fused_bce = pass == kTrain ? 1 : c.fused_bce;                // (the plan offers no train kernel without it)
  }
  if (pass == kBackward) { a.d_hidden = c.d_hidden; a.d_pos = c.d_pos; a.d_neg = c.d_neg; }
  if (pass != kTrain) { a.dbg = c.dbg; a.dbg_seq = c.dbg_seq; srfrd_debug_shape(c.lay, c.L, &a.dbg_slot, nullptr); }
  if (k.scratch_stride) { a.scratch = c.scratch; a.scratch_stride = k.scratch_stride; }
  switch (k.family) {
    case kFwdFirst: return launch_fwd_first(k, a, c.stream);
    case kFwdRows: return launch_fwd_rows(k, a, c.stream);
    case kFwdRagged: return launch_fwd_ragged(k, a, c.stream);
    case kFwdLong: return launch_fwd_long(k, &a, c.stream);
    case kBwdFirst: return launch_bwd_first(k, a, c.stream);
    case kBwdRagged: return launch_bwd_ragged(k, a, c.stream);
    case kBwdSlots: return launch_bwd_slots(k, a, c.stream);
    case kBwdChunks: return launch_bwd_chunks(k, a, c.stream);
    case kBwdLong: return launch_bwd_long(k, &a, c.stream);
    case kTrainRagged: return launch_train_ragged(k, a, c.stream);
  }
  return SRFRD_E_UNSUPPORTED;
}
}  // namespace srfrd

extern "C" int srfrd_encoder_fwd(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                                 const int64_t* input_ids, const int64_t* fake_ids, const int64_t* pos_ids,
                                 const int64_t* pos_fake, const int64_t* neg_ids, const int64_t* neg_fake, int B, int L,
                                 double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                                 float* hidden, float* pos_logits, float* neg_logits, float* save_x, float* save_h1,
                                 float* save_aux, float* loss_part, float* scratch, int64_t scratch_floats, float* dbg, int dbg_seq,
                                 void* stream) {
  EncCall c = {};
  c.lay = lay; c.item_table = item_table; c.dense = dense; c.packed = packed; c.input_ids = input_ids; c.fake_ids = fake_ids;
  c.pos_ids = pos_ids; c.pos_fake = pos_fake; c.neg_ids = neg_ids; c.neg_fake = neg_fake; c.B = B; c.L = L; c.dropout_p = dropout_p;
  c.seed = seed; c.seed_dev = seed_dev; c.seq_index0 = seq_index0; c.hidden = hidden; c.pos_logits = pos_logits; c.neg_logits = neg_logits;
  c.save_x = save_x; c.save_h1 = save_h1; c.save_aux = save_aux; c.loss_part = loss_part;
  c.scratch = scratch; c.scratch_floats = scratch_floats; c.dbg = dbg; c.dbg_seq = dbg_seq; c.stream = stream;
  return enc_run(c, kForward);
}

extern "C" int srfrd_encoder_fwd_sched(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                                       const int64_t* input_ids, const int64_t* fake_ids, const int64_t* pos_ids,
                                       const int64_t* pos_fake, const int64_t* neg_ids, const int64_t* neg_fake, int B, int L,
                                       double dropout_p, uint32_t seed, const uint32_t* seed_dev, int64_t seq_index0,
                                       float* hidden, float* pos_logits, float* neg_logits, float* save_x, float* save_h1,
                                       float* save_aux, float* loss_part, float* scratch, int64_t scratch_floats,
                                       const int32_t* sched, int sched_mode, void* stream) {
  if (!check_sched(sched, sched_mode)) return SRFRD_E_ARG;
  EncCall c = {};
  c.lay = lay; c.item_table = item_table; c.dense = dense; c.packed = packed; c.input_ids = input_ids; c.fake_ids = fake_ids;
  c.pos_ids = pos_ids; c.pos_fake = pos_fake; c.neg_ids = neg_ids; c.neg_fake = neg_fake; c.B = B; c.L = L; c.dropout_p = dropout_p;
  c.seed = seed; c.seed_dev = seed_dev; c.seq_index0 = seq_index0; c.hidden = hidden; c.pos_logits = pos_logits; c.neg_logits = neg_logits;
  c.save_x = save_x; c.save_h1 = save_h1; c.save_aux = save_aux; c.loss_part = loss_part;
  c.scratch = scratch; c.scratch_floats = scratch_floats; c.sched = sched; c.sched_mode = sched_mode; c.stream = stream;
  return enc_run(c, kForward);
}

extern "C" int srfrd_encoder_fwd_last(const srfrd_layout* lay, const void* item_table, const float* dense, const float* packed,
                                      const int64_t* input_ids, const int64_t* fake_ids, int B, int L, float* hidden_last,
                                      float* scratch, int64_t scratch_floats, void* stream) {
  EncCall c = {};
  c.lay = lay; c.item_table = item_table; c.dense = dense; c.packed = packed; c.input_ids = input_ids; c.fake_ids = fake_ids;
  c.B = B; c.L = L; c.hidden = hidden_last; c.last_only = 1; c.scratch = scratch; c.scratch_floats = scratch_floats; c.stream = stream;
  return enc_run(c, kForward);
}

extern "C" int srfrd_layout_init(srfrd_layout* lay, int kind, int n_items, int max_len, int d_item, int d_fake,
                                 int n_labels, int n_blocks, int n_heads) {
  if (!lay || kind < 0 || kind > SRFRD_SRFU_R || n_items < 1 || max_len < 1 || d_item < 1 || n_blocks < 1 ||
      n_blocks > SRFRD_MAX_BLOCKS || n_heads < 1)
    return SRFRD_E_ARG;
  const bool has_fake = kind == SRFRD_SRFR || kind == SRFRD_SRFRN;
  const bool is_srfu = kind >= SRFRD_SRFU_B;
  if (has_fake && d_fake < 1) return SRFRD_E_ARG;
  if (is_srfu && n_labels < 1) return SRFRD_E_ARG;
  srfrd_layout l = {};
  l.kind = kind; l.n_items = n_items; l.max_len = max_len; l.d_item = d_item;
  l.d_fake = has_fake ? d_fake : 0;
  l.D = d_item + l.d_fake;
  l.d_out = kind == SRFRD_SRFR ? d_item : l.D;
  l.n_labels = is_srfu ? n_labels : 0;
  l.n_blocks = n_blocks; l.n_heads = n_heads;
  if (l.D % n_heads != 0) return SRFRD_E_ARG;
  const int64_t D = l.D;
  int64_t off = 0;
  l.off_pos = off; off += (int64_t)max_len * d_item;
  l.side_rows = has_fake ? 3 : (is_srfu ? n_labels : 0);
  l.side_cols = has_fake ? d_fake : (is_srfu ? l.D : 0);
  l.off_side = off; off += (int64_t)l.side_rows * l.side_cols;
  for (int i = 0; i < n_blocks; ++i) {
    srfrd_block_off& o = l.blk[i];
    o.ln1_w = off; off += D; o.ln1_b = off; off += D;
    o.in_w = off; off += 3 * D * D; o.in_b = off; off += 3 * D;
    o.out_w = off; off += D * D; o.out_b = off; off += D;
    o.ln2_w = off; off += D; o.ln2_b = off; off += D;
    o.c1_w = off; off += D * D; o.c1_b = off; off += D;
    o.c2_w = off; off += D * D; o.c2_b = off; off += D;
  }
  if (kind == SRFRD_SRFR) {
    l.off_lc_w = off; off += (int64_t)d_item * D;
    l.off_lc_b = off; off += d_item;
  } else {
    l.off_lc_w = -1; l.off_lc_b = -1;
  }
  l.off_ll_w = off; off += l.d_out;
  l.off_ll_b = off; off += l.d_out;
  l.n_dense = off;
  l.n_table = (int64_t)(n_items + 1) * d_item;
  *lay = l;
  return 0;
}
