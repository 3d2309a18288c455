// The pieces the feature-space kernels share (neighbors.hip, kmeans.hip, tsne.hip, influence.hip, density.hip, laplace.hip): the scan of
// one feature row, the 32 x 32 tile of dot products on the exact-fp32 matrix instruction with the staging that feeds it, the distance of
// two rows from their norms and their dot product, and the Gram tiles of the upper triangle.  Several claims of DESIGN.md rest on these
// being ONE piece of code: the three consumers of a row agree on which rows exist, and a distance is the same bits in the search and in
// the assignment.
//
// v_mfma_f32_32x32x2_f32 is a k-ordered fp32 fma chain: one instruction adds a[m][0] b[0][n] and then a[m][1] b[1][n] to every element
// of a 32 x 32 accumulator tile, lane half 0 supplying k = 0 and lane half 1 k = 1.  Which FEATURE a lane half supplies in which step is
// a property of how the caller staged its rows, so every caller states the k-order its staging yields.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace ftile {

// ---- one feature row -------------------------------------------------------------------------------------------------------------------
// Row `row` of x (n, E), E a multiple of 4, rows 16-byte aligned: the squared norm (one fma chain in ascending feature index) goes to
// norm[row] (norm (n), or nullptr: not kept), and the row is good when every feature and the norm are finite and, with cosine, the norm
// is positive: ok[row] = 1, else 0.  With xhat (n, E) not null the unit row v / sqrt(norm) is written there, zeros for a row that is
// not good.  Returns good.
__device__ __forceinline__ bool row_scan(const float* x, float* norm, int* ok, float* xhat, int row, int E, bool cosine) {
  const int E4 = E / 4;
  const float4* src = reinterpret_cast<const float4*>(x + (size_t)row * E);
  float s = 0.f;
  bool fin = true;
  for (int c = 0; c < E4; ++c) {
    const float4 v = src[c];
    fin &= isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w);
    s = fmaf(v.x, v.x, s);
    s = fmaf(v.y, v.y, s);
    s = fmaf(v.z, v.z, s);
    s = fmaf(v.w, v.w, s);
  }
  const bool good = fin && isfinite(s) && (!cosine || s > 0.f);
  if (norm) norm[row] = s;
  ok[row] = good ? 1 : 0;
  if (xhat) {
    float4* dst = reinterpret_cast<float4*>(xhat + (size_t)row * E);
    const float len = sqrtf(s);
    for (int c = 0; c < E4; ++c) {
      const float4 v = src[c];
      dst[c] = good ? make_float4(v.x / len, v.y / len, v.z / len, v.w / len) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  return good;
}

// The counts of a row scan, a thread per row and whole waves calling: the good rows and the rows inside the table that are not good, one
// ballot each and one integer atomic per wave; the thread that owns row 0 writes n.  counts: 8-byte words, zeroed before the launch.
__device__ __forceinline__ void count_rows(unsigned long long* counts, bool good, int row, int n, int slot_n, int slot_valid, int slot_bad) {
  const unsigned long long m_good = __ballot(good), m_bad = __ballot(row < n && !good);
  if ((threadIdx.x & 63) == 0) {
    if (m_good) atomicAdd(&counts[slot_valid], (unsigned long long)__popcll(m_good));
    if (m_bad) atomicAdd(&counts[slot_bad], (unsigned long long)__popcll(m_bad));
  }
  if (row == 0) counts[slot_n] = (unsigned long long)n;
}

// ---- the pair tile ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ f32x16 mfma2(float a, float b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0); }

// register r of lane half lh of an accumulator tile holds row (r & 3) + 8 (r >> 2) + 4 lh of the tile; the column is lane & 31
__device__ __forceinline__ int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// acc[m][n] + sum over the columns [0, kend) of A[m][.] B[n][.], kend a multiple of 8: arow / brow point at column 4 (lane >> 5) of this
// lane's row (lane & 31) of A / B in LDS.  A lane half reads one float4 per group of 8 columns and the four instructions of the group
// take its .x .y .z .w in turn, so the chain of a pair runs through the columns as the staging laid them out.  (The accumulators of this
// file go in and out by value: a helper is optimised on its own before it is inlined, and one that updates them through a reference
// keeps them in memory there, which costs copies of the whole tile in the caller's loop.)
__device__ __forceinline__ f32x16 tile_dot(f32x16 acc, const float* arow, const float* brow, int kend) {
  for (int kk = 0; kk < kend; kk += 8) {
    const float4 a4 = *reinterpret_cast<const float4*>(arow + kk);
    const float4 b4 = *reinterpret_cast<const float4*>(brow + kk);
    acc = mfma2(a4.x, b4.x, acc);
    acc = mfma2(a4.y, b4.y, acc);
    acc = mfma2(a4.z, b4.z, acc);
    acc = mfma2(a4.w, b4.w, acc);
  }
  return acc;
}

// one unit = 8 consecutive features of one row: two float4 in, two float4 out as (f0 f2 f4 f6 | f1 f3 f5 f7), so that a lane half reads
// one float4 and the four matrix instructions of a group see k = (f0, f1), (f2, f3), ...: ascending.  The loops that fetch a tile's
// units and stage them stay with their kernels (knn_search_kernel, km_assign_kernel, inf_search_kernel).
__device__ __forceinline__ void store_unit(float* dst, const float4 u, const float4 v) {
  *reinterpret_cast<float4*>(dst) = make_float4(u.x, u.z, v.x, v.z);
  *reinterpret_cast<float4*>(dst + 4) = make_float4(u.y, u.w, v.y, v.w);
}

// the distance of two rows from their squared norms and their dot product (with cosine: of the unit rows): l2 = max(0, (xn + cn) - 2 dot),
// cosine = max(0, 1 - dot).  Norms near the top of the fp32 range can overflow the sum or the product: such a pair has no fp32 distance,
// *finite is false and the pair is no candidate.
__device__ __forceinline__ float dist_of(bool cosine, float xn, float cn, float dot, bool* finite) {
  const float raw = cosine ? 1.f - dot : (xn + cn) - 2.f * dot;
  *finite = isfinite(raw);
  return raw > 0.f ? raw : 0.f;
}

// ---- Gram tiles: X^T (w X) of the upper tile triangle --------------------------------------------------------------------------------
// A (P, P) Gram matrix, P = 32 T, is T (T + 1) / 2 tiles of 32 x 32 on and above the diagonal, numbered row-major.  The four waves of a
// workgroup share them round-robin: wave wv owns the tiles wv + 4 q, q < NQ = ceil(tiles / 4).

constexpr int upper_tiles(int T) { return T * (T + 1) / 2; }

// tile q of the upper triangle, row-major: (i, j), i <= j < T
__device__ __forceinline__ void upper_tile(int q, int T, int& i, int& j) {
  i = 0;
  while (q >= T - i) { q -= T - i; ++i; }
  j = i + q;
}

template <int T, int NQ>
__device__ __forceinline__ void wave_tiles(int wv, int (&ti)[NQ], int (&tj)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    ti[q] = tj[q] = 0;
    if (wv + 4 * q < upper_tiles(T)) upper_tile(wv + 4 * q, T, ti[q], tj[q]);
  }
}

// One slab of 32 rows, Xs [32][32 T] in LDS, added to the wave's tiles: the rows of the slab run along k of the matrix instruction in
// order, two per instruction.  The B operand of slab row k is b_of(k)(x), functors of the caller's: b_of(k) is taken once per row (the
// place for what depends on the row alone, a weight read from LDS for instance) and maps every element x of that row.
template <int T, int NQ, typename BOf>
__device__ __forceinline__ void gram_slab(f32x16 (&acc)[NQ], const float* Xs, int wv, const int (&ti)[NQ], const int (&tj)[NQ], BOf b_of) {
  constexpr int P = 32 * T;
  const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
  f32x16 c[NQ];                                                 // the tiles in registers for the length of the slab: see tile_dot
#pragma unroll
  for (int q = 0; q < NQ; ++q) c[q] = acc[q];
#pragma unroll 4
  for (int k2 = 0; k2 < 16; ++k2) {
    const float* xr = Xs + (2 * k2 + lh) * P + l31;             // row k, column l31 of a tile: conflict-free
    const auto b = b_of(2 * k2 + lh);
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (wv + 4 * q < upper_tiles(T)) c[q] = mfma2(xr[32 * ti[q]], b(xr[32 * tj[q]]), c[q]);
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = c[q];
}

// an accumulator tile to out [32][32]: column = lane & 31, row = acc_row(r, lane >> 5)
__device__ __forceinline__ void store_acc_tile(float* out, const f32x16& acc) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) out[acc_row(r, lh) * 32 + l31] = acc[r];
}

// element el of stored tile q is the Gram matrix' [ra][rb], and [rb][ra] by symmetry; true for the elements below the diagonal of a
// diagonal tile, which are the mirror of those above it and are skipped
__device__ __forceinline__ bool fold_element(int q, int el, int T, int& ra, int& rb) {
  const int m = el >> 5, nn = el & 31;
  int i, j;
  upper_tile(q, T, i, j);
  ra = 32 * i + m;
  rb = 32 * j + nn;
  return i == j && m > nn;
}

}  // namespace ftile
