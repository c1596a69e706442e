// Kernel plan of full-catalog ranking: which kernels srfrd_logits_topk(_excl) and srfrd_target_rank launch for a (layout,
// op, B, k, item range, exclusion, switch set), in order, with the grid, block and dynamic LDS of each.  Host only: the plan
// makes no HIP call (srfrd_rank_plan asks it on a machine without a GPU).  rank_plan (srfrd_rank.hip) is the one place
// that chooses and the one place that refuses; the launchers launch what it names.
#pragma once
#include <stdint.h>

#include "../../include/srfrd_hip.h"

namespace srfrd {

enum RankKernel {
  kExclPrep,         // excl_prep_kernel
  kTopkMax16,        // topk_max16_kernel<nu, !table_bf16, excl>
  kTopkCollect16,    // topk_collect16_kernel<nu, !table_bf16>
  kTopkMax,          // topk_max_kernel<excl>
  kTopkTau,          // topk_tau_kernel
  kTopkCollect,      // topk_collect_kernel
  kTopkExclFilter,   // topk_excl_filter_kernel
  kTopkSelect,       // topk_select_kernel
  kTopkStage1,       // topk_stage1_kernel<excl>
  kTopkStage2,       // topk_stage2_kernel
  kTargetScore16,    // target_score16_kernel<!table_bf16>
  kTargetScore,      // target_score_kernel
  kTargetCount16,    // target_count16_kernel<nu, !table_bf16, excl>
  kTargetCount,      // target_count_kernel<excl>
  kTargetMetric,     // target_metric_kernel
};

struct RankLaunch {
  int kernel;        // RankKernel
  int grid, block;
  int64_t lds;       // dynamic LDS bytes
};

struct RankPlan {
  int rc;            // 0, or SRFRD_E_UNSUPPORTED: the call refuses before its first launch
  bool stream16;     // the bf16 matrix-core streams (else the fp32 stream)
  bool split_e;      // stream16 over an fp32 table (three bf16 planes per row)
  bool excl;         // the masked instantiations
  int nu;            // stream16: user tiles per wave
  int crows;         // rows of one chunk of the stream: 256, or 512 on stream16 over a bf16 table
  int stream_chunks; // chunks of the stream (the stride of the chunk maxima)
  int wg_per_group;  // stream16: persistent workgroups per user group
  int user_splits;   // fp32 stream: workgroups per chunk
  int n_chunks;      // 256-row chunks: the workspace offsets and the exhaustive path
  int n_launches;
  RankLaunch launch[8];
};

// op: SRFRD_RANK_* (include/srfrd_hip.h), switches: SRFRD_SW_* bits (read_switches), n_cu: CUs of the device.  The
// arguments are ones the entry point accepted (B > 0, 1 <= k <= 64 for top-k, 0 <= item_lo < item_hi).
RankPlan rank_plan(const srfrd_layout& lay, int op, int B, int k, int64_t item_lo, int64_t item_hi, bool excl, int switches,
                   int n_cu);

}  // namespace srfrd
