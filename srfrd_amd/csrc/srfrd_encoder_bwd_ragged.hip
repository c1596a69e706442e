// Ragged fused encoder backward at the reference's default geometry (srfrd_encoder_bwd_ragged_kernel.inc): the autograd pass
// behind `loss.backward()` (reference trainer.py:40) computed on the rows a left-padded sequence really has, reading the
// checkpoints of the ragged forward.  srfrd_encoder_bwd (srfrd_encoder_bwd.hip) dispatches here when the kernel plan (encoder_plan) pairs the ragged kernels.
#include "srfrd_enc_common.h"

#include "srfrd_encoder_fwd_ragged_kernel.inc"      // kRagSH, rag_take (the forward kernel template itself is not instantiated here)
#include "srfrd_encoder_bwd_ragged_kernel.inc"

namespace srfrd {

int launch_bwd_ragged(const KernelPlan& k, const EncArgs& a, void* stream) {
  return with_variant_flag(k, [&](auto K, auto DI, auto rmw) { return launch_enc(encoder_bwd_ragged_kernel<K, DI, rmw>, k, stream, a); });
}

}  // namespace srfrd
