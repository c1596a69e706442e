// Long-sequence build of the fused encoder fwdward pass: the same kernel source with the per-sequence working set
// in a global-memory scratch (SRFRD_BUF_GLOBAL) instead of LDS, for shapes that do not fit 160 KiB.
#define SRFRD_BUF_GLOBAL 1
#include "srfrd_enc_common.h"
#include "srfrd_encoder_fwd_kernel.inc"

#include <cstring>

namespace srfrd {

// args: the caller's srfrd::EncArgs (identical layout); the plan sized scratch / scratch_stride and the LDS share
int launch_fwd_long(const KernelPlan& k, const void* args, void* stream) {
  srfrd_long::EncArgs a;
  std::memcpy(&a, args, sizeof(a));
  a.lds_floats = (int)(k.lds / 4);      // as much of the working set as fits goes to LDS (flat addressing), the rest to scratch
  const auto kernel = srfrd_long::encoder_fwd_kernel<0, 0, 0>;
  if (const int rc = lds_opt_in((const void*)kernel, srfrd_long::kLdsLimit)) return rc;
  hipLaunchKernelGGL(kernel, dim3(k.grid), dim3(k.threads), (size_t)k.lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace srfrd
