/*
 * srfrd_hip_sort.h  --  the device key sort of libsrfrd_hip.so: the third public header of the C ABI, beside srfrd_hip.h and
 * srfrd_hip_lazy.h.  The conventions of srfrd_hip.h (device pointers, caller-owned buffers, stream-ordered and
 * graph-capturable launches, return codes) hold here word for word.
 *
 * Every sorted train step ends in one stable sort of item-id keys (DESIGN sections 18, 23 and 24).  This is that sort as
 * kernels of the library's own: a least-significant-digit radix sort over the 16 to 20 bits an item id has, ceil(bits / 8)
 * passes over 4-byte keys.  The call enqueues kernel launches and nothing else - no memset, no allocation, no copy - so a
 * graph may hold it at any length.
 */
#ifndef SRFRD_HIP_SORT_H
#define SRFRD_HIP_SORT_H

#include "srfrd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of workspace srfrd_sort_keys needs for n keys in [0, key_max] (host only: no device is touched).  Positive for
 * every accepted (n, key_max), n == 0 included, and non-decreasing in n and in key_max: a workspace sized for the longest
 * list and the largest table serves every shorter list.  0: refused - n < 0, n > INT_MAX, key_max < 0 or
 * key_max > 2^31 - 3.
 */
int64_t srfrd_sort_keys_workspace_bytes(int64_t n, int64_t key_max);

/*
 * The stable sort of n int64 keys.  The sort key of a key is
 *   u(key) = 0            if key < 0
 *          = key + 1      if 0 <= key <= key_max
 *          = key_max + 2  if key > key_max
 * so every invalid id lands at one of the two ends of the list, where srfrd_table_reduce and its kin skip it; no address is
 * ever computed from a key's value.  On completion
 *   order        is a permutation of [0, n);
 *   u(keys[order[j]]) is non-decreasing in j, and equal u appear in ascending order[j]  (stable);
 *   sorted_keys[j] == keys[order[j]], the original 64-bit value.
 * With every key in [0, key_max] that is exactly torch.sort(keys, stable=True): there is one correct output, and this is it,
 * bit for bit, on every call.
 *
 * bits = bit length of (key_max + 2); passes = ceil(bits / 8) of ceil(bits / passes) <= 8 bits each (50 001 table rows: 2
 * passes; 1 M rows: 3).  A pass is three launches (count, scan, scatter); a workgroup never waits for another workgroup of
 * its launch.  keys is only read.  workspace: ws_bytes >= srfrd_sort_keys_workspace_bytes(n, key_max) bytes on a 16-byte
 * boundary, the call's alone while it runs; its contents before the call do not matter and nothing in it needs zeroing.
 *
 * SRFRD_E_ARG before any launch: keys, sorted_keys, order or workspace NULL; n < 0 or n > INT_MAX; key_max < 0 or
 * key_max > 2^31 - 3; ws_bytes below the query's answer; workspace not 16-byte aligned; sorted_keys or order equal to keys,
 * or equal to each other.  n == 0 returns 0 and launches nothing (the refusals come first).
 */
int srfrd_sort_keys(const int64_t* keys, int64_t n, int64_t key_max,
                    int64_t* sorted_keys, int64_t* order,
                    void* workspace, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRFRD_HIP_SORT_H */
