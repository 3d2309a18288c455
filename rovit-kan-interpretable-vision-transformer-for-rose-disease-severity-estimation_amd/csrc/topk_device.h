// Ascending lists of 64-bit keys, the top-k building blocks of the searches (neighbors.hip, influence.hip) and of the assignment
// (kmeans.hip): a key is (orderable value bits << 32) | row index, the k smallest keys win, and only integer compares decide membership.
// Here: the key itself, the per-lane list, the merge of the four lists a query tile's waves hold for one query, and the plan that
// splits the reference rows of a search over work items.
#pragma once
#include "common.h"

namespace topk {

typedef unsigned long long u64;

constexpr u64 EMPTY = ~0ull;                     // above every real key: its value bits would be a NaN's

__device__ __forceinline__ u64 key_of(unsigned bits, int j) { return ((u64)bits << 32) | (u64)(unsigned)j; }
__device__ __forceinline__ unsigned key_bits(u64 c) { return (unsigned)(c >> 32); }
__device__ __forceinline__ int key_index(u64 c) { return (int)(unsigned)(c & 0xffffffffull); }

// the number of keys below c in an ascending list of KB keys (KB a power of two)
__device__ __forceinline__ int keys_below(const u64* list, int KB, u64 c) {
  int lo = 0;
  for (int s = KB >> 1; s > 0; s >>= 1)
    if (list[lo + s - 1] < c) lo += s;
  return lo + (list[lo] < c ? 1 : 0);
}

template <int KB>
__device__ __forceinline__ void list_insert(u64 (&lst)[KB], u64 key) {
  if (key < lst[KB - 1]) {
    lst[KB - 1] = key;
#pragma unroll
    for (int i = KB - 1; i > 0; --i) {
      const u64 lo = lst[i - 1], hi = lst[i];
      const bool swap = hi < lo;
      lst[i - 1] = swap ? hi : lo;
      lst[i] = swap ? lo : hi;
    }
  }
}

// The four lists of every query of a 64-query tile (two lane halves, two waves) meet in Ms [64][4][KB]: this lane's list goes to list
// `slot` (= 4 query + list); then thread (query tid >> 2, list tid & 3) ranks its list's keys: a key's rank among the four is its index
// in its own list plus a binary search in the three others, and the KB smallest go to out, the KB words of query tid >> 2 (nullptr: that
// query does not exist).  The first barrier is there because Ms lies over the caller's staging buffers (and over an earlier call's lists).
template <int KB>
__device__ __forceinline__ void merge_four(const u64 (&lst)[KB], u64* Ms, int slot, u64* out) {
  const int tid = threadIdx.x;
  __syncthreads();
  {
    u64* mine = Ms + slot * KB;
#pragma unroll
    for (int i = 0; i < KB; ++i) mine[i] = lst[i];
  }
  __syncthreads();
  const int ql = tid >> 2, li = tid & 3;
  if (out) {
    const u64* base = Ms + ql * 4 * KB;
    for (int i = 0; i < KB; ++i) {
      const u64 c = base[li * KB + i];
      if (c == EMPTY) break;
      int rank = i;
      for (int o = 0; o < 4; ++o)
        if (o != li) rank += keys_below(base + o * KB, KB, c);
      if (rank < KB) out[rank] = c;
    }
    if (li == 0) {
      int real = 0;
      for (int o = 0; o < 4; ++o) real += keys_below(base + o * KB, KB, EMPTY);
      for (int s = real; s < KB; ++s) out[s] = EMPTY;
    }
  }
}

// ---- host: the plan of a search ------------------------------------------------------------------------------------------------------
// A work item = (tile of 64 queries, split of the 64-row reference tiles).  The splits are chosen to reach two work items per CU, at most
// 64 of them and at most max_splits when that is positive; kb is the list length that serves k.

inline int bucket_of(int k) { return k <= 8 ? 8 : (k <= 16 ? 16 : 32); }

struct Plan { int qtiles, rtiles, splits, tps, kb; };
inline Plan plan_of(int B, int N, int k, int max_splits) {
  constexpr int TILE = 64, TARGET_ITEMS = 512, MAX_SPLITS = 64;
  Plan p;
  p.qtiles = (B + TILE - 1) / TILE;
  p.rtiles = (N + TILE - 1) / TILE;
  p.kb = bucket_of(k);
  long long s = (TARGET_ITEMS + p.qtiles - 1) / p.qtiles;
  s = s < 1 ? 1 : s;
  s = s > MAX_SPLITS ? MAX_SPLITS : s;
  s = (max_splits > 0 && s > max_splits) ? max_splits : s;
  s = s > p.rtiles ? p.rtiles : s;
  p.tps = (p.rtiles + (int)s - 1) / (int)s;
  p.splits = (p.rtiles + p.tps - 1) / p.tps;      // never more than without the cap: the default workspace serves every cap
  return p;
}

}  // namespace topk
