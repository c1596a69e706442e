/*
 * srfrd_hip_lazy.h  --  the lazy-Adam entry point of libsrfrd_hip.so: the second public header of the C ABI, beside
 * srfrd_hip.h, whose conventions (device pointers, caller-owned buffers, stream-ordered and graph-capturable launches,
 * return codes) hold here word for word.
 *
 * Lazy Adam is a different optimizer for an embedding table, not a faster form of the dense one (TensorFlow's LazyAdam, the
 * row-wise half of torch.optim.SparseAdam): a row's moments and value are stepped only on the steps whose batch names the
 * row, with the GLOBAL step's bias correction.  A row nobody named keeps its bits - it is not dragged along by its stale
 * momentum - and the table's share of a step costs in proportion to the batch, not to the catalog.
 */
#ifndef SRFRD_HIP_LAZY_H
#define SRFRD_HIP_LAZY_H

#include "srfrd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * From the sorted row keys of a batch straight to the stepped rows: srfrd_table_reduce and srfrd_adam_step on the rows the
 * batch touches, as one launch, without the table gradient in between.
 *
 * sorted_keys / order / table_contrib / n / d_item: as srfrd_table_reduce (n keys sorted ascending by a STABLE sort,
 * order[j] = the contribution row sorted position j came from, d_item floats per row).  table, m, v: the item table and its
 * Adam moments, n_rows rows of d_item floats each.  For every key k that heads a run of equal keys, 1 <= k < n_rows:
 *   g[c]  = sum over the run, in ascending sorted position j, of table_contrib[order[j] * d_item + c]
 *           (one fp32 chain from 0.f: the bits srfrd_table_reduce stores)
 *   g    *= gscale,  gscale = 1 / stats[2] if stats != NULL else 1                        (as srfrd_adam_step)
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= step_size * m / (sqrt(v) / bc2_sqrt + eps)   on row k of m, v, table,
 *           step_size = state[4], bc2_sqrt = state[5]: srfrd_adam_step's arithmetic, instruction for instruction, so a
 *           touched row gets the bits srfrd_table_reduce into a zeroed gradient + srfrd_adam_step would give it
 *   table_bf16 (may be NULL): row k of the bf16 shadow = the stepped values rounded to nearest even.
 * Everything else is left alone: key 0 (padding_idx) is skipped; a key outside [1, n_rows) is skipped and never
 * dereferenced; a row whose key does not occur is neither read nor written, in table, m, v and table_bf16 alike.  order[j]
 * is trusted to index table_contrib, as in srfrd_table_reduce.
 *
 * `state` is READ (words 4 and 5, as srfrd_step_begin / srfrd_step_begin_sched left them) and NOT advanced: the caller
 * enqueues this call BEFORE the launch that advances it (srfrd_adam_pack_step / srfrd_adamw_pack_step over the dense
 * parameters, or srfrd_step_begin for the next step).  Under a schedule the words are the scheduled ones; the decay word
 * state[7] is not read (lazy Adam runs without weight decay).
 *
 * SRFRD_E_ARG before any launch: sorted_keys, order, table_contrib, table, m, v or state NULL; n < 0; d_item outside
 * 1..64; n_rows < 1.  n == 0 returns 0 and launches nothing.
 */
int srfrd_table_reduce_adam(const int64_t* sorted_keys, const int64_t* order, const float* table_contrib,
                            int64_t n, int d_item, int64_t n_rows,
                            float* table, float* m, float* v,
                            double beta1, double beta2, double eps,
                            const uint32_t* state, const float* stats,
                            uint16_t* table_bf16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRFRD_HIP_LAZY_H */
