// The (key u64, value u32) sort that otto_events.hip defines and the pair and feature builders share (kernels: radix.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Stable sort of n (key u64, value u32) pairs by key, in the workspace of otto_events_sort_workspace(n): d_keys must be
// the workspace's first key buffer; on return *d_keys_sorted / *d_vals_sorted point INTO the workspace.
int otto_sort_pairs_in_ws(uint64_t* d_keys, int64_t n, void* d_ws, uint64_t** d_keys_sorted, uint32_t** d_vals_sorted, hipStream_t s);
// pointers of the first (key, value) buffers and the scan scratch inside a sort workspace
void otto_sort_ws_buffers(int64_t n, void* d_ws, uint64_t** key0, uint32_t** val0, uint64_t** scan_out, uint64_t** scan_partial);
