// Long-sequence build of the fused encoder bwdward pass: the same kernel source with the per-sequence working set
// in a global-memory scratch (SRFRD_BUF_GLOBAL) instead of LDS, for shapes that do not fit 160 KiB.
#define SRFRD_BUF_GLOBAL 1
#include "srfrd_enc_common.h"
#include "srfrd_encoder_bwd_kernel.inc"

#include <cstring>

namespace srfrd {

template <class K>
static int launch_long(K kernel, const KernelPlan& k, const srfrd_long::EncArgs& a, void* stream) {
  if (const int rc = lds_opt_in((const void*)kernel, srfrd_long::kLdsLimit)) return rc;
  hipLaunchKernelGGL(kernel, dim3(k.grid), dim3(k.threads), (size_t)k.lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

// args: the caller's srfrd::EncArgs (identical layout); the plan sized scratch / scratch_stride and the LDS share.
// kL100: SASRec, hidden 50, seq_len 100, fused training step (BASELINE configs[3] geometry) - compile-time shape
int launch_bwd_long(const KernelPlan& k, const void* args, void* stream) {
  srfrd_long::EncArgs a;
  std::memcpy(&a, args, sizeof(a));
  a.lds_floats = (int)(k.lds / 4);      // as much of the working set as fits goes to LDS (flat addressing), the rest to scratch
  if (k.form == kL100) return launch_long(srfrd_long::encoder_bwd_kernel<50, 112, 8, 100, SRFRD_SASREC, 1, 50>, k, a, stream);
  return launch_long(srfrd_long::encoder_bwd_kernel<0, 0, 0>, k, a, stream);
}

}  // namespace srfrd
