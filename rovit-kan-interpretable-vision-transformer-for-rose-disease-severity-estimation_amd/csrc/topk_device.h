// Per-lane ascending lists of 64-bit keys, the top-k building blocks of the searches (neighbors.hip, influence.hip): a key is
// (orderable value bits << 32) | row index, the k smallest keys win, and only integer compares decide membership.
#pragma once
#include "common.h"

namespace topk {

typedef unsigned long long u64;

constexpr u64 EMPTY = ~0ull;                     // above every real key: its value bits would be a NaN's

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

// one unit = 8 consecutive features of one row: two float4 in, two float4 out as (f0 f2 f4 f6 | f1 f3 f5 f7), so that a lane half reads
// one float4 and the four matrix instructions of a group see k = (f0, f1), (f2, f3), ...: ascending
__device__ __forceinline__ void store_unit(float* dst, const float4 u, const float4 v) {
  *reinterpret_cast<float4*>(dst) = make_float4(u.x, u.z, v.x, v.z);
  *reinterpret_cast<float4*>(dst + 4) = make_float4(u.y, u.w, v.y, v.w);
}

}  // namespace topk
