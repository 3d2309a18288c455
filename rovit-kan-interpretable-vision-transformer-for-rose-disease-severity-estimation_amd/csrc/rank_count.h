// The tile of the counting rank of sel_rank_kernel (selective.hip) and ood_rank_kernel (density.hip); eval_rank_count_kernel (evaluate.hip)
// ranks two columns per pass and keeps the same two loops written out over both (see there).  A thread owns one x_i; the x_j are staged
// in LDS RANK_RT at a time and every lane reads the same address (a broadcast: no bank conflict); less = #{x_j < x_i} and
// eq = #{x_j == x_i} are exact uint32 counts.  O(n^2) by choice: exact, order-free, no sort.
// Which columns share a pass, how a work item maps to (chunk, split, column), the barriers around the staging and the integer atomics
// that add the counts of a split j range stay with the kernels.
#pragma once
#include <hip/hip_runtime.h>

constexpr int RANK_RT = 1024;           // x_j per LDS tile
constexpr int RANK_NT = 256;            // threads per workgroup the staging loop is written against; the kernels assert their NT

// sX[k] = X[j0 + k] for the j0 + k < lim, NaN behind them: NaN is neither below nor equal to anything, so the padding counts nothing.
// The caller puts a barrier before (the previous tile's readers) and after.
__device__ __forceinline__ void rank_stage_tile(float* sX, const float* __restrict__ X, int j0, int lim) {
  for (int k = threadIdx.x; k < RANK_RT; k += RANK_NT) sX[k] = j0 + k < lim ? X[j0 + k] : __builtin_nanf("");
}

// Adds one staged tile's counts for xi.  BEFORE: also *before += #{k < d : sX[k] == xi}, the equal AND earlier x_j of a tile that
// straddles the thread's own row (d = i - j0); a tile wholly before or behind the workgroup's rows needs no index compare.
template <bool BEFORE = false>
__device__ __forceinline__ void rank_count_tile(const float* sX, float xi, unsigned& less, unsigned& eq, unsigned* before = nullptr, int d = 0) {
#pragma unroll 4
  for (int k = 0; k < RANK_RT / 4; ++k) {
    const float4 v = reinterpret_cast<const float4*>(sX)[k];
    less += (v.x < xi) + (v.y < xi) + (v.z < xi) + (v.w < xi);
    eq += (v.x == xi) + (v.y == xi) + (v.z == xi) + (v.w == xi);
    if (BEFORE) {
      const int k4 = 4 * k;
      *before += ((v.x == xi) & (k4 < d)) + ((v.y == xi) & (k4 + 1 < d)) + ((v.z == xi) & (k4 + 2 < d)) + ((v.w == xi) & (k4 + 3 < d));
    }
  }
}

// The same counting rank of a short list of 32-bit words held whole in LDS (patch_dropout.hip: 196 Philox words per sample), by the
// integer pair (word, index): rank_i = #{j : w_j < w_i or (w_j == w_i and j < i)}.  Ties are broken by the index, so the ranks are a
// permutation of 0..n-1 whatever the words are.  Integer compares only; every lane reads the same address (a broadcast).
__device__ __forceinline__ unsigned rank_count_pairs_u32(const unsigned* sW, int n, unsigned wi, int i) {
  unsigned rank = 0;
#pragma unroll 4
  for (int j = 0; j < n; ++j) {
    const unsigned wj = sW[j];
    rank += (wj < wi) | ((wj == wi) & (j < i));
  }
  return rank;
}
