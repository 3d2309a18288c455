// The augmented hidden rows of one 64-row tile of a head, a = [relu(fc1 f + b1); 1; 0 ...]: ONE set of device functions for the Laplace
// kernels (laplace.hip) and the whitened last-layer gradients (influence.hip), so the two files cannot drift apart.
// Definitions: include/rovit_hip.h, the Laplace comment.
#pragma once
#include "common.h"

namespace laplace {

constexpr int NT = 256;                 // threads per workgroup
constexpr int MAXC = ROVIT_EVAL_MAX_CLASSES;
constexpr int ROWS = ROVIT_LAPLACE_TILE;
static_assert(ROWS == 64, "two row tiles of 32 per workgroup");

// Fs [64][E + 4]: the staged feature rows; As [64][P + 4] receives relu(fc1 f + b1) in columns 0 .. hid - 1, 1 in column hid, zeros up to
// P; a row whose s_ok is 0 is zero throughout.  The product is accumulated in fp64 on the vector unit, one fma chain over e in order,
// and rounded to fp32 ONCE after the bias and the ReLU: the hidden row is the correctly rounded one.  (An fp32 chain on the matrix
// instruction, even split four ways, left the Gram matrices of a handful of rows up to 4.4 times the error of a blocked fp32 sum: the
// hidden row's error is the only one that no later sum averages out.  fc1 is hid x E x 64 fma a tile, a small share of either kernel.)
// Thread (rg, jg): rows rg, rg + 16, rg + 32, rg + 48 (16 bytes a step each: conflict-free at a row stride of E + 4), columns 2 jg and
// 2 jg + 1 of every 32-column pass; fc1 is read from memory (every workgroup reads the same hid x E words: they stay in L2).  No barrier
// inside: the caller puts one before (Fs, s_ok) and one after (As).  A NaN passes the ReLU (h < 0 is false), as torch.relu lets it.
__device__ __forceinline__ void lap_hidden(const float* Fs, float* As, const int* s_ok, const float* __restrict__ w1,
                                           const float* __restrict__ b1, int E, int hid) {
  const int ST = E + 4, SA = hid + 36;
  const int tid = threadIdx.x, rg = tid & 15, jg = tid >> 4;
  for (int j0 = 0; j0 < hid; j0 += 32) {
    const int j = j0 + 2 * jg;
    const float* wa = w1 + (size_t)j * E;
    const float* wb = wa + E;
    double acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = 0.0;
    for (int e = 0; e < E; e += 4) {
      const float4 u = *reinterpret_cast<const float4*>(wa + e);
      const float4 v = *reinterpret_cast<const float4*>(wb + e);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 f = *reinterpret_cast<const float4*>(Fs + (rg + 16 * i) * ST + e);
        acc[i][0] = fma((double)f.x, (double)u.x, acc[i][0]);
        acc[i][0] = fma((double)f.y, (double)u.y, acc[i][0]);
        acc[i][0] = fma((double)f.z, (double)u.z, acc[i][0]);
        acc[i][0] = fma((double)f.w, (double)u.w, acc[i][0]);
        acc[i][1] = fma((double)f.x, (double)v.x, acc[i][1]);
        acc[i][1] = fma((double)f.y, (double)v.y, acc[i][1]);
        acc[i][1] = fma((double)f.z, (double)v.z, acc[i][1]);
        acc[i][1] = fma((double)f.w, (double)v.w, acc[i][1]);
      }
    }
    const double ba = (double)b1[j], bb = (double)b1[j + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rg + 16 * i;
      const bool ok = s_ok[row] != 0;
      double ha = acc[i][0] + ba, hb = acc[i][1] + bb;
      ha = ha < 0.0 ? 0.0 : ha;
      hb = hb < 0.0 ? 0.0 : hb;
      As[row * SA + j] = ok ? (float)ha : 0.f;
      As[row * SA + j + 1] = ok ? (float)hb : 0.f;
    }
  }
  for (int idx = tid; idx < ROWS * 32; idx += NT) {             // the 1 and the padding
    const int r = idx >> 5, c = idx & 31;
    As[r * SA + hid + c] = (c == 0 && s_ok[r] != 0) ? 1.f : 0.f;
  }
}

__device__ __forceinline__ void lap_stage_features(float* Fs, const float* __restrict__ x, int r0, int n, int E) {
  const int E4 = E / 4, ST = E + 4;
  for (int idx = threadIdx.x; idx < ROWS * E4; idx += NT) {
    const int row = idx / E4, c4 = idx - row * E4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row < n) v = *reinterpret_cast<const float4*>(x + (size_t)(r0 + row) * E + 4 * c4);
    *reinterpret_cast<float4*>(Fs + row * ST + 4 * c4) = v;
  }
}

// As [64][SA], then a region that holds the feature rows first and the two W tiles afterwards (SA = hid + 36), in floats
__host__ __device__ inline size_t lap_stream_region(int E, int hid) {
  const size_t SA = hid + 36;
  return (size_t)ROWS * (E + 4) > 64 * SA ? (size_t)ROWS * (E + 4) : 64 * SA;
}

}  // namespace laplace
