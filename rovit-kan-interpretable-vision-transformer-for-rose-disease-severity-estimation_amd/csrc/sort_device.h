// The device radix sort of fp32 columns (sort_rank.hip) as the other files see it: the order-preserving key, the two binary searches
// over a sorted key array that turn it into the counted ranks of rank_count.h, and the host entry points the consumers of a rank
// (evaluate.hip, selective.hip, density.hip) launch.  Definitions: include/rovit_hip.h, the rovit_sort comment; DESIGN.md section 2.
#pragma once
#include "common.h"

constexpr unsigned ROVIT_SORT_NAN_KEY = 0xFFFFFFFFu;       // behind +inf (0xFF800000); no number has this key
constexpr int ROVIT_SORT_SEARCH_STEPS = 21;                // halvings that empty an interval of n <= 2^20 slots: floor(log2 n) + 1

#ifdef __HIPCC__

// the order-preserving key of an fp32 value (numbers only), and back
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ unsigned key_bits(unsigned k) { return (k >> 31) ? k ^ 0x80000000u : ~k; }

// The sort's key of ANY fp32 value: order_key(v + 0.0f), so -0 shares +0's key, and every NaN (either sign, any payload) gets
// ROVIT_SORT_NAN_KEY.  Written on the bits: v + 0.0f differs from v for -0 only.
__device__ __forceinline__ unsigned sort_key(float v) {
  const unsigned b = __float_as_uint(v);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return ROVIT_SORT_NAN_KEY;
  return b == 0x80000000u ? 0x80000000u : b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// First slot of the ascending keys s[0, n) whose key is >= k (lower) or > k (upper); n when there is none.  mid < hi <= n, so
// every read is inside the array; the loop ends after ROVIT_SORT_SEARCH_STEPS halvings whatever the memory holds.
__device__ __forceinline__ unsigned lower_bound(const unsigned* __restrict__ s, unsigned n, unsigned k) {
  unsigned lo = 0, hi = n;
  for (int it = 0; it < ROVIT_SORT_SEARCH_STEPS && lo < hi; ++it) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (s[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ unsigned upper_bound(const unsigned* __restrict__ s, unsigned n, unsigned k) {
  unsigned lo = 0, hi = n;
  for (int it = 0; it < ROVIT_SORT_SEARCH_STEPS && lo < hi; ++it) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (s[mid] <= k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

#endif  // __HIPCC__

// ---- host side (internal, not part of the C ABI) ----------------------------------------------------------------------------------
// One column of a batched sort: keys[n] and perm[n] receive the ascending (key, row) pairs.  The callers have checked pointers and sizes.
struct RovitSortCol { const float* x; unsigned* keys; unsigned* perm; int n; };
size_t rovit_sort_batch_workspace_bytes(const int* n, int cols);          // 0 outside the limits
int rovit_sort_batch(const RovitSortCol* c, int cols, void* workspace, size_t workspace_bytes, int max_workgroups, hipStream_t stream,
                     const char* who);
// less[i] = #{sorted < x_i}, eq[i] = #{sorted == x_i} for the n rows of x against the m sorted keys of a column (its own or another);
// a NaN row gets 0 and 0.
struct RovitRankQuery { const float* x; int n; const unsigned* sorted; int m; unsigned* less; unsigned* eq; };
int rovit_rank_search(const RovitRankQuery* q, int queries, int max_workgroups, hipStream_t stream, const char* who);
// less, eq and before of every row of a sorted column, written at the row each sorted slot holds (before: the slot minus less)
struct RovitRankSlots { const unsigned* keys; const unsigned* perm; int n; unsigned* less; unsigned* eq; unsigned* before; };
int rovit_rank_slots(const RovitRankSlots* c, int cols, int max_workgroups, hipStream_t stream, const char* who);
// ROVIT_RANK_AUTO resolved for n rows
static inline int rovit_rank_method(int method, long long n) {
  return method == ROVIT_RANK_AUTO ? (n >= ROVIT_RANK_SORT_ROWS ? ROVIT_RANK_SORT : ROVIT_RANK_COUNT) : method;
}
