/*
 * srfrd_hip_topk_wide.h  --  exact full-catalog top-k for k up to 1024: the fourth public header of the C ABI of
 * libsrfrd_hip.so, beside srfrd_hip.h, whose conventions (device pointers, caller-owned buffers, stream-ordered and
 * graph-capturable launches, return codes) hold here word for word.
 *
 * srfrd_logits_topk(_excl) stop at k = 64: their threshold is the k-th largest maximum of a 256- or 512-row chunk, their
 * candidate list holds 2048 entries and their selection is k argmax rounds.  A re-ranker's candidate pull, Recall@100 / @200
 * or a page that must survive business filters want hundreds of items; the wide call gives them without the (B, n_items)
 * logits ever reaching memory.  Nothing about the k <= 64 entry points changes.
 */
#ifndef SRFRD_HIP_TOPK_WIDE_H
#define SRFRD_HIP_TOPK_WIDE_H

#include "srfrd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRFRD_TOPK_WIDE_MAX 1024      /* largest k of srfrd_logits_topk_wide */

/* the path of a wide plan (sizes[0] of srfrd_topk_wide_plan) */
#define SRFRD_WIDE_FINE 0     /* threshold from group maxima finer than a chunk (a lane's strip of a run of 16-row tiles) */
#define SRFRD_WIDE_CHUNK 1    /* threshold from the chunk maxima: the k <= 64 ranking's own first pass, as it is */
#define SRFRD_WIDE_ALL 2      /* no threshold (tau = -inf): the item range has at most `capacity` rows, every one collects */

/*
 * [host] the kernel plan of srfrd_logits_topk_wide, asked without a GPU (no HIP call): the launches of one call, in order,
 * reported as srfrd_rank_plan reports them - names + i * name_len receives launch i's kernel as a kernel trace prints it
 * ("srfrd::wide_collect16_kernel<2,true>", at most name_len bytes with the NUL), geom[3 i .. 3 i + 2] its workgroups, threads
 * per workgroup and dynamic LDS bytes; at most max_launches launches are written (8 hold every plan); names and geom may be
 * NULL.  sizes (3 int32, may be NULL) receives {path (SRFRD_WIDE_*), candidate capacity per user, group maxima per user}.
 * excl != 0: the call carries an exclusion set.  switches: SRFRD_SW_* bits (the call itself reads them from the environment),
 * n_cu: compute units of the device.
 *
 * Every plan ends in wide_select_kernel and wide_fallback_kernel: the fallback is launched by every call and its workgroups
 * leave at once unless their user's candidate list overflowed.
 *
 * Returns the number of launches; SRFRD_E_ARG for lay NULL, B <= 0, k outside 1..SRFRD_TOPK_WIDE_MAX, a bad item range
 * (item_lo < 0, item_hi <= item_lo, item_hi > n_items + 1), n_cu <= 0 or max_launches < 0; SRFRD_E_UNSUPPORTED exactly
 * where srfrd_logits_topk_wide would return it: every such refusal of the call is this function's, made before a launch.
 */
int srfrd_topk_wide_plan(const srfrd_layout* lay, int B, int k, int64_t item_lo, int64_t item_hi, int excl, int switches,
                         int n_cu, int max_launches, char* names, int name_len, int32_t* geom, int32_t* sizes);

/*
 * [host] bytes of the `workspace` of srfrd_logits_topk_wide for B users, k and an item range of n_rows rows (group maxima,
 * thresholds, cursors and B lists of `capacity` 8-byte candidates); it depends on nothing else, so one buffer serves every
 * layout and switch set.  0 where the call would refuse these values: B <= 0, k outside 1..SRFRD_TOPK_WIDE_MAX, n_rows <= 0.
 */
int64_t srfrd_topk_wide_workspace_bytes(int B, int k, int64_t n_rows);

/*
 * srfrd_logits_topk_excl for 1 <= k <= SRFRD_TOPK_WIDE_MAX, with that call's semantics word for word: the score of item i for
 * user b is <hidden[b, L - 1, :d_item], table[i]> (+ SRFRN's side term), over {i in [item_lo, item_hi) : i not in excl[b],
 * !(exclude_pad && i == 0)}; the bf16 shadow is read when lay->table_bf16 is set; d_item > 52 and the SRFRD_TOPK_FP32 switch
 * take the fp32 stream.  The scores come from the k <= 64 ranking's own stream code, so they have its bits.
 *   topk_idx (B, k) int64, topk_val (B, k) fp32: values descending, equal values by ascending id; the slots behind the last
 *   rankable item hold -1 / -inf.  Exact for any input, every score tied included.
 *   excl_ptr == NULL: no exclusion sets (excl_items, max_row and excl_workspace are then not read).  Otherwise the CSR of
 *   srfrd_logits_topk_excl with excl_workspace of srfrd_excl_workspace_bytes(B, max_row, n_rows) bytes.
 *   workspace / ws_bytes: at least srfrd_topk_wide_workspace_bytes(B, k, item_hi - item_lo) bytes; contents need not be
 *   initialised and are not kept between calls.
 *
 * Launches: what srfrd_topk_wide_plan names (with read switches and the device's CU count), on `stream`, in order - the
 * exclusion pre-pass if any, the group maxima, the thresholds, the collection, the per-user sort, the fallback.  No host
 * synchronisation and no memset: cursors and overflow counts are reset by the threshold kernel, so the call can be captured
 * in a graph and replayed.  A user whose candidates overflow the capacity (mass ties at the threshold) gets its whole list
 * from the fallback - one workgroup streaming the range, fp64 accumulation rounded once, values within the bound of the
 * streams' - and every other user's list keeps the bits it would have had without that user in the batch.
 *
 * SRFRD_E_ARG before any launch: lay, item_table, dense, hidden, topk_idx, topk_val or workspace NULL; user_label NULL for
 * SRFRN; B <= 0, L <= 0; k outside 1..SRFRD_TOPK_WIDE_MAX; item_lo < 0, item_hi <= item_lo or item_hi > n_items + 1; ws_bytes
 * below the query; with excl_ptr: excl_items or excl_workspace NULL, max_row < 0.  SRFRD_E_UNSUPPORTED before any launch:
 * max_row > SRFRD_EXCL_CAP (and srfrd_logits_topk_excl's 32-bit limits), D > SRFRD_MAX_D, and what the plan refuses.
 */
int srfrd_logits_topk_wide(const srfrd_layout* lay, const void* item_table, const float* dense, const float* hidden,
                           int B, int L, int64_t item_lo, int64_t item_hi, int exclude_pad, const int64_t* user_label,
                           int k, const int64_t* excl_ptr, const int32_t* excl_items, int max_row,
                           int64_t* topk_idx, float* topk_val, void* workspace, int64_t ws_bytes, void* excl_workspace,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRFRD_HIP_TOPK_WIDE_H */
