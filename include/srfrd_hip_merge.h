/*
 * srfrd_hip_merge.h  --  merge of sorted top-k lists of up to SRFRD_TOPK_WIDE_MAX entries: the sixth public header of the C ABI
 * of libsrfrd_hip.so, beside srfrd_hip.h, whose conventions (device pointers, caller-owned buffers, stream-ordered and
 * graph-capturable launches, return codes) hold here word for word.
 *
 * Every ranking call returns each user's list sorted by the order law - values descending, equal values by ascending id, -0 as
 * +0 - with the empty slots (-1 / -inf) trailing.  The lists one user gets from the shards of a row-sharded catalog are sorted
 * runs, and srfrd_topk_merge_runs merges them as runs: srfrd_topk_merge selects k times among at most 4096 candidates, this
 * call finishes a sorting network that the runs have already begun, over up to 16 384.  Nothing about the
 * other entry points changes.
 */
#ifndef SRFRD_HIP_MERGE_H
#define SRFRD_HIP_MERGE_H

#include "srfrd_hip_topk_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * [host] dynamic LDS bytes of wide_merge_kernel for n_lists lists of list_len slots: 8 P with P = pow2ceil(n_lists) *
 * pow2ceil(list_len) keys of 8 bytes, or 0 where srfrd_topk_merge_runs refuses these two values (either below 1, or
 * P > 16 384).  No HIP call.
 */
int64_t srfrd_topk_merge_runs_lds_bytes(int n_lists, int list_len);

/*
 * The best k of n_lists candidate lists per user, by the order law.
 *   cand_idx int64, cand_val fp32: slot j of list s of user b is element b * user_stride + s * list_stride + j of both (strides
 *   in elements).  An (n_lists, B, list_len) stack - what a loop over shards stacks up, what an all-to-all delivers - merges in
 *   place with user_stride = list_len, list_stride = B * list_len; a (B, n_lists * list_len) concatenation with user_stride =
 *   n_lists * list_len, list_stride = list_len.
 *   cand_idx < 0: an empty slot, its value is not read.  Ids are below 2^31 - 1024, the ranking's own limit.
 *   topk_idx (B, k) int64, topk_val (B, k) fp32: values descending, equal values by ascending id, -0 written as +0; the slots
 *   behind the last candidate hold -1 / -inf.  Every slot is written (a dirty buffer is fine).
 *   path (B) int32, or NULL (not written): 0 - the user's lists were sorted runs and were merged; 1 - one of them was not and
 *   all of the user's candidates were sorted.
 *
 * Semantics.  A valid id with value -inf is a candidate: it sorts behind every finite value and before the empty slots.  Equal
 * ids in two lists are both kept: shards are disjoint, the call does not deduplicate.  NaN takes the place the order-preserving
 * key gives it (a positive NaN above +inf, a negative one below -inf), as in srfrd_logits_topk_wide's selection; no caller
 * produces one.
 *
 * Exact for any input: while a workgroup loads its user's lists it tests every neighbouring pair of a list; a list that is not
 * sorted by the order law, empty slots last, sends the user to the full sort, whose result does not depend on the order of the
 * candidates - as srfrd_topk_merge's does not.
 *
 * One launch (wide_merge_kernel: one workgroup of 1024 threads per user, srfrd_topk_merge_runs_lds_bytes of dynamic LDS):
 * no workspace, no memset, no host synchronisation; the call can be captured on one stream and replayed.
 *
 * SRFRD_E_ARG before any launch: cand_idx, cand_val, topk_idx or topk_val NULL; B, n_lists or list_len < 1; k outside
 * 1..SRFRD_TOPK_WIDE_MAX; strides under which two slots of a user alias: list_stride < list_len with more than one list, or
 * user_stride < 1.  SRFRD_E_UNSUPPORTED before any launch: pow2ceil(n_lists) * pow2ceil(list_len) > 16 384 (128 KiB of keys:
 * the ceiling of the wide selection's own sort).
 */
int srfrd_topk_merge_runs(const int64_t* cand_idx, const float* cand_val, int B, int n_lists, int list_len,
                          int64_t user_stride, int64_t list_stride, int k,
                          int64_t* topk_idx, float* topk_val, int32_t* path, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRFRD_HIP_MERGE_H */
