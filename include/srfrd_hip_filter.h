/*
 * srfrd_hip_filter.h  --  item filters (allow masks) for exact full-catalog top-k and target rank: the fifth public header
 * of the C ABI of libsrfrd_hip.so, beside srfrd_hip.h, whose conventions (device pointers, caller-owned buffers,
 * stream-ordered and graph-capturable launches, return codes) hold here word for word.
 *
 * srfrd_logits_topk_wide and srfrd_target_rank restrict the catalog by a contiguous item range and by a per-user exclusion
 * set of at most SRFRD_EXCL_CAP ids.  "Only items in stock", "only this category", "this tenant's slice" are large arbitrary
 * subsets shared by many users: a packed bitmap over the item ids, one row per group of users.  The calls below rank over
 *   {i in [item_lo, item_hi) : allow[g(b)][i], i not in excl[b], !(exclude_pad && i == 0)}
 * with the scores of the unfiltered calls, bit for bit: a disallowed score turns to -inf inside the stream pass, before it
 * reaches a maximum, a candidate list or a count.  Nothing about the other entry points changes.
 */
#ifndef SRFRD_HIP_FILTER_H
#define SRFRD_HIP_FILTER_H

#include "srfrd_hip_topk_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * [host] 32-bit words of one bitmap row over the ids 0 .. n_rows - 1: W = (n_rows + 31) / 32 + 1.  Bit (i & 31) of word
 * (i >> 5) belongs to the absolute item id i; the last word and every bit at or past n_rows are zero, so a two-word window
 * at any id stays inside the row.  0 for n_rows <= 0.  No HIP call.
 */
int64_t srfrd_item_mask_words(int64_t n_rows);

/*
 * mask (n_groups, n_rows) bytes, nonzero = allowed  ->  words (n_groups, srfrd_item_mask_words(n_rows)) uint32, every word
 * written (a dirty buffer is fine), the last word and the tail bits zero.  One launch (item_mask_pack_kernel: a wave ballot per
 * 64 items, no atomics) on `stream`; capturable.
 * SRFRD_E_ARG before any launch: mask or words NULL, n_groups < 1, n_rows < 1.  SRFRD_E_UNSUPPORTED before any launch:
 * n_rows >= 2^31 - 1024 (the ranking's own limit on an id).
 */
int srfrd_item_mask_pack(const uint8_t* mask, int n_groups, int64_t n_rows, uint32_t* words, void* stream);

/*
 * [host] the kernel plan of srfrd_logits_topk_allow, asked without a GPU (no HIP call), in the form of srfrd_topk_wide_plan:
 * names + i * name_len receives launch i's kernel as a kernel trace prints it ("srfrd::allow_collect16_kernel<true,false>": the
 * template arguments are SPLIT_E - an fp32 table on the bf16 stream - and EXCL - the call carries exclusion sets), geom[3 i ..
 * 3 i + 2] its workgroups, threads per workgroup and dynamic LDS bytes; at most max_launches launches are written (8 hold every
 * plan); names and geom may be NULL.  sizes (3 int32, may be NULL) receives {path, candidate capacity per user, group maxima
 * per user}.
 *
 * The threshold is the k-th largest maximum of groups of at most r item rows with k r <= capacity, so a filtered call overflows a
 * candidate list only through exact ties of group maxima at the threshold, whatever the filter looks like:
 *   SRFRD_WIDE_ALL   the item range has at most `capacity` rows: no maxima, tau = -inf, every allowed finite score collects;
 *   SRFRD_WIDE_FINE  bf16 stream: a lane quarter's strip of 2^t 16-row tiles of a 256-row chunk, the largest t <= 4 with
 *                    4 2^t k <= capacity (64 rows up to k = 256, 32 at 512, 16 at 1024); fp32 stream: the 8 rows a lane
 *                    quarter of one wave owns of a 256-row chunk (32 groups per chunk).
 * SRFRD_WIDE_CHUNK is never chosen: the unfiltered chunk maxima are not maxima of the allowed items.  The stream passes run
 * at the geometry of the masked k <= 64 plan (one user tile per wave, 256-row chunks) with or without exclusion sets.
 * Every plan ends in wide_select_kernel and allow_fallback_kernel, whose workgroups leave at once unless their user's
 * candidate list overflowed.
 *
 * Returns the number of launches; SRFRD_E_ARG for lay NULL, B <= 0, k outside 1..SRFRD_TOPK_WIDE_MAX, a bad item range
 * (item_lo < 0, item_hi <= item_lo, item_hi > n_items + 1), n_cu <= 0 or max_launches < 0; SRFRD_E_UNSUPPORTED exactly
 * where srfrd_logits_topk_allow would return it: every such refusal of the call is this function's, made before a launch.
 */
int srfrd_topk_allow_plan(const srfrd_layout* lay, int B, int k, int64_t item_lo, int64_t item_hi, int excl, int switches,
                          int n_cu, int max_launches, char* names, int name_len, int32_t* geom, int32_t* sizes);

/*
 * [host] bytes of the `workspace` of srfrd_logits_topk_allow for B users, k and an item range of n_rows rows: 32 group maxima
 * per 256 rows and user (the fp32 stream's; about 125 k floats per user at a million rows), thresholds, cursors, B lists of
 * `capacity` 8-byte candidates and 4 maxima per 256 rows and user for the collection pass's skip test.  It depends on nothing
 * else.  0 where the call would refuse these values: B <= 0, k outside 1..SRFRD_TOPK_WIDE_MAX, n_rows <= 0.  No HIP call.
 */
int64_t srfrd_topk_allow_workspace_bytes(int B, int k, int64_t n_rows);

/*
 * srfrd_logits_topk_wide over the allowed items, with that call's semantics word for word otherwise: 1 <= k <=
 * SRFRD_TOPK_WIDE_MAX (k <= 64 included), the bf16 shadow when lay->table_bf16 is set, d_item > 52 and the SRFRD_TOPK_FP32 switch
 * on the fp32 stream, exclude_pad, excl_ptr == NULL for no exclusion sets.
 *   allow_words (n_groups, words_per_group) uint32: rows packed by srfrd_item_mask_pack over the ids 0 .. n_items (words_per_group
 *   may exceed srfrd_item_mask_words(n_items + 1); the words behind it are not read).
 *   allow_group (B) int64: the bitmap row of user b, clamped into [0, n_groups) as every id is; NULL: every user reads row 0.
 *   topk_idx (B, k) int64, topk_val (B, k) fp32: values descending, equal values by ascending id; the slots behind the last
 *   allowed rankable item hold -1 / -inf (a filter that allows nothing gives all -1 / -inf).  Exact for any input, every score
 *   tied included.
 *   workspace / ws_bytes: at least srfrd_topk_allow_workspace_bytes(B, k, item_hi - item_lo) bytes, contents not kept.
 *
 * Launches: what srfrd_topk_allow_plan names, on `stream`, in order - the exclusion pre-pass if any, the masked group maxima
 * (none on SRFRD_WIDE_ALL), wide_tau_kernel, the masked collection, wide_select_kernel, allow_fallback_kernel.  No host
 * synchronisation and no memset: the threshold kernel resets the cursors, so the call can be captured on one stream and
 * replayed.  A user whose candidates overflow the capacity gets its whole list from the fallback workgroup (fp64 accumulation
 * rounded once, the bit tested beside the exclusion set); every other user's list keeps its bits.
 *
 * SRFRD_E_ARG before any launch: everything srfrd_logits_topk_wide refuses with it (lay, item_table, dense, hidden, topk_idx,
 * topk_val or workspace NULL; user_label NULL for SRFRN; B <= 0, L <= 0; k outside 1..SRFRD_TOPK_WIDE_MAX; a bad item range;
 * ws_bytes below the query; with excl_ptr: excl_items or excl_workspace NULL, max_row < 0); allow_words NULL; n_groups < 1;
 * words_per_group < srfrd_item_mask_words(n_items + 1).  SRFRD_E_UNSUPPORTED before any launch: max_row > SRFRD_EXCL_CAP (and
 * srfrd_logits_topk_excl's 32-bit limits), D > SRFRD_MAX_D, and what the plan refuses.
 */
int srfrd_logits_topk_allow(const srfrd_layout* lay, const void* item_table, const float* dense, const float* hidden,
                            int B, int L, int64_t item_lo, int64_t item_hi, int exclude_pad, const int64_t* user_label,
                            int k, const int64_t* excl_ptr, const int32_t* excl_items, int max_row,
                            int64_t* topk_idx, float* topk_val, void* workspace, int64_t ws_bytes, void* excl_workspace,
                            const uint32_t* allow_words, int n_groups, int64_t words_per_group, const int64_t* allow_group,
                            void* stream);

/*
 * srfrd_target_rank over the allowed items: rank[b] = #{i in [item_lo, item_hi) : i != t_b, allow[g(b)][i], i not in excl[b],
 * !(exclude_pad && i == 0), s(b, i) > s(b, t_b)}.  The target's score comes from srfrd_target_rank's own score kernel: the target
 * is ranked even when the filter disallows it, exactly as an excluded target is, and bit-identical copies of its row are never
 * counted.  Ranks over disjoint item ranges add up.  cut_k / metric_acc: as srfrd_target_rank (metric_acc NULL: no metric
 * launch).  workspace: srfrd_excl_workspace_bytes(B, max_row, item_hi - item_lo) bytes (max_row 0 without sets).
 *
 * Launches: the exclusion pre-pass if any, target_score16_kernel / target_score_kernel, allow_count16_kernel /
 * allow_count_kernel at the masked plan's geometry, target_metric_kernel if asked.  No host synchronisation: capturable.
 *
 * SRFRD_E_ARG before any launch: everything srfrd_target_rank refuses with it (targets, rank or workspace NULL, cut_k <= 0, the
 * shared arguments as above); allow_words NULL; n_groups < 1; words_per_group < srfrd_item_mask_words(n_items + 1).
 * SRFRD_E_UNSUPPORTED before any launch: as srfrd_target_rank with an exclusion set.
 */
int srfrd_target_rank_allow(const srfrd_layout* lay, const void* item_table, const float* dense, const float* hidden,
                            int B, int L, int64_t item_lo, int64_t item_hi, int exclude_pad, const int64_t* user_label,
                            const int64_t* targets, const int64_t* excl_ptr, const int32_t* excl_items, int max_row,
                            int cut_k, int32_t* rank, double* metric_acc, void* workspace,
                            const uint32_t* allow_words, int n_groups, int64_t words_per_group, const int64_t* allow_group,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRFRD_HIP_FILTER_H */
