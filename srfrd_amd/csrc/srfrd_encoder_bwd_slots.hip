// Slot-placed, query-chunked fused encoder backward (srfrd_encoder_bwd_slots_kernel.inc): the LDS-resident backward of
// the fused training step at seq_len 100 (BASELINE configs[3]); srfrd_encoder_bwd (srfrd_encoder_bwd.hip) dispatches
// here when shape and mode qualify, every other long-sequence case runs the global-scratch build.
#include "srfrd_enc_common.h"

#include "srfrd_encoder_bwd_slots_kernel.inc"

namespace srfrd {

int launch_bwd_slots(const KernelPlan& k, const EncArgs& a, void* stream) {
  return with_variant_flag(k, [&](auto K, auto DI, auto rmw) {
    return k.form == kL50 ? launch_enc(encoder_bwd_slots_kernel<50, 50, K, DI, rmw>, k, stream, a)
                          : launch_enc(encoder_bwd_slots_kernel<50, 100, K, DI, rmw>, k, stream, a);
  });
}

}  // namespace srfrd
