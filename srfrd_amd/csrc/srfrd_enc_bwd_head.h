// What the four encoder backward kernel sources share of a sequence's HEAD - the part of its backward that runs before the
// block loop.  Included by srfrd_enc_common.h inside each build's namespace (srfrd / srfrd_long get their own copy).
//
// Users: srfrd_encoder_bwd_kernel.inc ("first", both namespaces), srfrd_encoder_bwd_slots_kernel.inc ("slots"),
// srfrd_encoder_bwd_chunks_kernel.inc ("chunks"), srfrd_encoder_bwd_ragged_kernel.inc ("ragged", also the backward half of
// the one-launch train kernel, whose forward head calls bce_dlogits too).
//
// Only what leaves EVERY kernel's instruction stream as it was is here (profiles/bwd_head_resources.txt):
//   HeadRow / kHeadRows   the order and the count of the per-position arrays: all four, the seam hand-off, the host LDS sizes
//   bce_dlogits           first, slots, chunks, ragged, the train kernel's forward head
//   head_zero_cols        slots, chunks (first: its one copy stays, the call reorders three instantiations; ragged: step 3)
// The id pass, the pass-1 gather, the pass-2 scatter, side_sums, SRFRN's fake term and the packed-weight lambda stay written
// out per family.  Moved into a function - forced or ordinary inlining, arguments by value or by reference, geometry as
// template or run-time arguments, a closure-like struct - each of them compiles to the same instructions in another order
// with other registers and spill counts, in every instantiation that executes it; so does a struct of the nine pointers
// built by a constructor wherever LP is a run-time value (chunks, the generic first-generation kernel) and in the train
// kernel.  Only text in the kernel body, or a lambda defined there, reproduces the schedule.  DESIGN.md, "The backward
// kernels' shared head", has the list of what was tried.
//
// No function here contains a workgroup barrier or launders an index.  head_zero_cols' parameters, each for a difference
// between its users: buf - the first of `rows` rows (slots: the sequence's L rows; chunks: a chunk's rows).
#pragma once

namespace SRFRD_NS {

// The per-position arrays every backward keeps at the front of its LDS tail: array k at tail + k * LP (ids as lds_i, the rest
// as lds_f).  A family places its own arrays (s_delta, s_brep, s_dummy) and s_misc from kHeadRows on; the host-side LDS sizes
// (srfrd_enc_common.h) count kHeadRows + the family's own.
enum HeadRow {
  kRowIn,      // clamped input id
  kRowKeep,    // 1 where the input id is not padding
  kRowPid, kRowNid,            // clamped target ids
  kRowFk, kRowPfk, kRowNfk,    // fake ids of the input and the targets
  kRowDpl, kRowDnl,            // logit gradients
  kHeadRows
};

// The fused masked BCE's logit gradients (trainer.py:36-38: both terms indexed by pos != 0): one definition for every
// backward's id pass and the train kernel's forward head (SEAM_), so that all contract the same way.
__device__ __forceinline__ void bce_dlogits(int pid, float pl, float nl, float& dp, float& dn) {
  if (pid != 0) {
    dp = sigmoid_f(pl) - 1.0f;
    dn = sigmoid_f(nl);
  }
}

// channels d_out..D-1 of `rows` rows of a gradient matrix are zero (SRFR: the last LayerNorm is d_out wide)
__device__ __forceinline__ void head_zero_cols(lds_f* buf, int DS, int rows, int dout, int D, int tid, int nthr) {
  if (dout < D)
    for (int idx = tid; idx < rows * (D - dout); idx += nthr) {
      const int tt = idx / (D - dout), cc = dout + idx - tt * (D - dout);
      buf[tt * DS + cc] = 0.f;
    }
}

}  // namespace SRFRD_NS
