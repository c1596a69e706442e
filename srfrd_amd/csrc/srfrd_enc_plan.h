// Kernel plan of the fused encoder: which instantiation srfrd_encoder_fwd / srfrd_encoder_bwd launch for a (layout, B, L,
// mode, switch set), with its grid, LDS and scratch stride.  Host only: the plan makes no HIP call (srfrd_encoder_plan asks
// it on a machine without a GPU).  encoder_plan (srfrd_encoder_fwd.hip) is the one place that chooses; the launchers
// launch what it names.
#pragma once
#include <stdint.h>

#include "../../include/srfrd_hip.h"

namespace srfrd {

enum Family {
  kFwdFirst,     // first-generation LDS kernel, srfrd_encoder_fwd_kernel.inc
  kFwdRows,      // row-owner forward, srfrd_encoder_fwd_rows_kernel.inc
  kFwdRagged,    // ragged forward, srfrd_encoder_fwd_ragged_kernel.inc
  kFwdLong,      // global-scratch build of the first-generation forward (srfrd_long::)
  kBwdFirst,     // first-generation LDS kernel, srfrd_encoder_bwd_kernel.inc
  kBwdRagged,    // ragged backward, srfrd_encoder_bwd_ragged_kernel.inc
  kBwdSlots,     // slot-placed backward, srfrd_encoder_bwd_slots_kernel.inc
  kBwdChunks,    // row-chunked backward, srfrd_encoder_bwd_chunks_kernel.inc
  kBwdLong,      // global-scratch build of the first-generation backward (srfrd_long::)
  kTrainRagged,  // ragged forward + backward in one launch, srfrd_encoder_train_ragged.hip
};

// Geometry template of the first-generation kernels (and the sequence length of the slot-placed backward)
enum Form {
  kGeneric,      // <0, 0, 0>: run-time geometry
  kLP32,         // <50, 32, 8>
  kLP64,         // <50, 64, 8>
  kL50,          // <50, 64, 8, 50, K, T, DI>, or <50, 64, 8, 50> without a kind variant
  kL100,         // SASRec at seq_len 100: <50, 112, 16 | 8, 100, SASREC, T, 50>
};

// Kind variants of the hidden-50, one-head specialisations: 0 SASRec 50 + 0, 1 SRFR 45 + 5, 2 SRFRN 45 + 5, 3 SRFU_* 50 + 0
// (kind read at run time) - the <K, DI> template arguments of every specialised kernel.
struct KindVariant {
  int K, DI;
};
constexpr KindVariant kKindVariants[4] = {{SRFRD_SASREC, 50}, {SRFRD_SRFR, 45}, {SRFRD_SRFRN, 45}, {-1, 50}};

struct KernelPlan {
  int rc;                  // 0, or SRFRD_E_UNSUPPORTED: no kernel serves this call (the launcher returns it)
  int family;              // Family
  int form;                // Form (first-generation, global-scratch and slot-placed families)
  int variant;             // kKindVariants index, or -1
  bool flag;               // the family's boolean template argument: training instantiation (first-generation, ragged
                           // forward), not plain eval (row-owner), read-modify-write slabs (ragged / slots / chunks backward)
  int grid, threads;
  int64_t lds;             // dynamic LDS bytes
  int64_t scratch_stride;  // floats of the caller's scratch per workgroup (global-scratch builds, row-chunked backward), or 0
};
struct EncPlan {
  KernelPlan fwd, bwd;
  KernelPlan train;        // a training forward and its fused-BCE backward as ONE launch (srfrd_encoder_train_sched), or rc set
};

// One call of a launching entry point (srfrd_encoder_fwd* / _bwd* / _train_*), its arguments by name: what the entry point
// does not take stays zero.  Host only, never a kernel argument: enc_run builds the kernels' EncArgs from it.
struct EncCall {
  const srfrd_layout* lay;
  const void* item_table;
  const float *dense, *packed;
  const int64_t *input_ids, *fake_ids, *pos_ids, *pos_fake, *neg_ids, *neg_fake;
  int B, L;
  double dropout_p;
  uint32_t seed;
  const uint32_t* seed_dev;
  int64_t seq_index0;
  float *hidden, *pos_logits, *neg_logits, *save_x, *save_h1, *save_aux;   // the forward writes them, the backward reads them
  float* loss_part;
  const float *d_hidden, *d_pos, *d_neg;     // upstream gradients (the train pass takes none)
  int fused_bce;
  float *grad_table, *table_contrib, *grad_slabs, *scratch;
  int64_t scratch_floats;
  float* dbg;
  int dbg_seq, last_only;
  const int32_t* sched;
  int sched_mode, rank_G;    // rank_G: srfrd_encoder_train_ranked's pair stride
  bool demand_scratch;       // srfrd_encoder_train_sched: srfrd_train_scratch_floats or more, once the plan has a kernel
  void* stream;
};
enum Pass { kForward, kBackward, kTrain };
// The one path from a call to a launch (srfrd_encoder_fwd.hip): the shared refusals, the pass's own, the plan, the launch.
// An entry point makes its own check (check_sched, the ranked step's pair stride), names its arguments and calls this.
int enc_run(const EncCall& c, Pass pass);
inline bool check_sched(const int32_t* sched, int sched_mode) { return sched_mode == 0 || (sched_mode == 1 && sched); }
// a layout the fused kernels cover (enc_run and the plan queries answer SRFRD_E_UNSUPPORTED otherwise)
inline bool layout_supported(const srfrd_layout& lay) {
  return lay.D <= SRFRD_MAX_D && lay.n_heads >= 1 && lay.D % lay.n_heads == 0 && lay.n_blocks <= SRFRD_MAX_BLOCKS &&
         (lay.flags & ~SRFRD_LAYOUT_MASK_PAD_KEYS) == 0;
}

// mode: SRFRD_PLAN_* bits, switches: SRFRD_SW_* bits (read_switches), n_cu: CUs of the device, scratch_floats: the caller's
// scratch (0 when none).  The layout is one layout_supported accepts.
EncPlan encoder_plan(const srfrd_layout& lay, int B, int L, int mode, int switches, int n_cu, int64_t scratch_floats);
// the instantiation's name as a kernel trace prints it (without spaces), e.g. "srfrd::encoder_fwd_ragged_kernel<0,1,50>"
void plan_name(const KernelPlan& k, char* buf, int len);
// persistent workgroups of the backward (= rows of grad_slabs): a function of the layout and the shape only
int bwd_grid(const srfrd_layout& lay, int B, int L, int n_cu);

int launch_fwd_long(const KernelPlan& k, const void* args, void* stream);   // srfrd_encoder_fwd_long.hip (args: EncArgs)
int launch_bwd_long(const KernelPlan& k, const void* args, void* stream);   // srfrd_encoder_bwd_long.hip

}  // namespace srfrd
