// Row-chunked fused encoder backward (srfrd_encoder_bwd_chunks_kernel.inc): the LDS-resident backward of the fused training
// step at seq_len 101..208 (BASELINE configs[4] trains at seq_len 200); srfrd_encoder_bwd dispatches here when shape and mode
// qualify and the caller's scratch holds the three [L][50] intermediates per workgroup.
#include "srfrd_enc_common.h"

#include "srfrd_encoder_bwd_chunks_kernel.inc"

namespace srfrd {

int launch_bwd_chunks(const KernelPlan& k, const EncArgs& a, void* stream) {
  return with_variant_flag(k, [&](auto K, auto DI, auto rmw) { return launch_enc(encoder_bwd_chunks_kernel<50, K, DI, rmw>, k, stream, a); });
}

}  // namespace srfrd
