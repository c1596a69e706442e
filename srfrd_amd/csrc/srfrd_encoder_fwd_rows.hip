// Row-owner inference forward for long sequences (srfrd_encoder_fwd_rows_kernel.inc): eval-mode hidden states (all
// positions, or the last one for ranking) at seq_len 113..208 - BASELINE configs[4] (seq_len 200) - with K / V resident in
// LDS; srfrd_encoder_fwd / srfrd_encoder_fwd_last dispatch here when shape and mode qualify, every other long-sequence
// case (training, target logits, debug taps) runs the global-scratch build.
#include "srfrd_enc_common.h"

#include "srfrd_encoder_fwd_rows_kernel.inc"

namespace srfrd {

int launch_fwd_rows(const KernelPlan& k, const EncArgs& a, void* stream) {
  return with_variant_flag(k, [&](auto K, auto DI, auto mode) { return launch_enc(encoder_fwd_rows_kernel<50, K, DI, mode>, k, stream, a); });
}

}  // namespace srfrd
