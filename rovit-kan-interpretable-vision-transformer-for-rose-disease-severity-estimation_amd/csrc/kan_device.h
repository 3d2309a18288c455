// Device helpers shared by the KAN / head kernels (kan_heads.hip, kan_stack.hip, head_phase.hip, kan_stats.hip, kan_grid.hip,
// explain.hip): the truncated cubic B-spline basis of /root/reference/models/kan.py:8-44 -- in closed form where the stored knots
// around the interval are uniform, by the recursion itself where they are not -- and the activations KANSeverityModule applies
// (:138-149).
#pragma once
#include "common.h"

namespace {

constexpr int KAN_MAX_KNOTS = 64;

struct Basis4 {
  int j;        // knot interval, -1 when every basis value is zero (beyond the truncation / saturated)
  float v[4];   // value of basis j-m, m = 0..3
};

// Knot interval of an already clamped coordinate xc: a guess from the uniform spacing, then an exact search on the stored knots.
// The one search of this file: kan_basis and kan_interval both call it.
__device__ __forceinline__ int kan_search(float xc, const float* knots, int nk, float t0, float inv_h0) {
  int j = (int)floorf((xc - t0) * inv_h0);
  j = j < 0 ? 0 : (j > nk - 1 ? nk - 1 : j);
  while (j > 0 && xc < knots[j]) --j;                          // exact search on the stored knots
  while (j < nk - 1 && xc >= knots[j + 1]) ++j;
  return j;
}

// Spans within this fraction of each other count as one uniform step: the package's own rule for a uniform grid
// (rovit_hip/kan_grid.py check_grid, models/kan.py _uniform_knots), so every grid those accept takes the closed form here as it
// does in km_basis (kan_stack.hip).
constexpr float KAN_UNIFORM_RTOL = 1e-4f;

// True when the five knot spans around interval j (the ones the four cubics alive on it depend on) all equal h within
// KAN_UNIFORM_RTOL h: then the closed form in u = (x - k_j) / h stands for the reference's recursion.  Spans off the left end do
// not count: the basis functions they would shape do not exist (kan.py:23-25).
__device__ __forceinline__ bool kan_locally_uniform(const float* knots, int j, float h) {
  float dev = 0.f;
#pragma unroll
  for (int m = -2; m <= 2; ++m) {
    if (m == 0) continue;
    const int a = j + m < 0 ? 0 : j + m;                       // j + 3 <= nk - 2 for a live interval (j < nk - 4)
    const float d = j + m < 0 ? h : knots[a + 1] - knots[a];
    dev = fmaxf(dev, fabsf(d - h));
  }
  return dev <= KAN_UNIFORM_RTOL * h;
}

// The four cubics alive on interval j of ANY strictly increasing knot vector, by the local form of the Cox-de Boor recursion the
// reference runs (kan.py:28-42): v[m] = basis j - m, dv[m] its slope.  Knot indices below 0 are clamped to 0: they enter only the
// basis functions of negative index, which the caller drops.
template <bool DERIV>
__device__ __forceinline__ void kan_basis_general(float x, const float* knots, int j, float* v, float* dv) {
  const float l1 = x - knots[j], l2 = x - knots[j >= 1 ? j - 1 : 0], l3 = x - knots[j >= 2 ? j - 2 : 0];
  const float r1 = knots[j + 1] - x, r2 = knots[j + 2] - x, r3 = knots[j + 3] - x;
  const float a = 1.f / (r1 + l1);                             // degree 1
  const float n10 = r1 * a, n11 = l1 * a;
  const float b0 = n10 / (r1 + l2), b1 = n11 / (r2 + l1);      // degree 2
  const float q0 = r1 * b0, q1 = l2 * b0 + r2 * b1, q2 = l1 * b1;
  const float c0 = q0 / (r1 + l3), c1 = q1 / (r2 + l2), c2 = q2 / (r3 + l1);   // degree 3
  v[3] = r1 * c0;
  v[2] = l3 * c0 + r2 * c1;
  v[1] = l2 * c1 + r3 * c2;
  v[0] = l1 * c2;
  if (DERIV) {
    dv[3] = -3.f * c0;
    dv[2] = 3.f * (c0 - c1);
    dv[1] = 3.f * (c1 - c2);
    dv[0] = 3.f * c2;
  }
}

// knots: LDS or global pointer to nk fp32 knots.  The STORED values are used for the interval search and for the basis, as the
// reference does (kan.py:24,33-38): the closed form where the knots around the interval are uniform (every grid the package builds),
// the recursion itself where they are not.
template <bool DERIV>
__device__ __forceinline__ Basis4 kan_basis(float xn, const float* knots, int nk, float inv_h0, float* dv) {
  Basis4 r;
  const int nb = nk - 4;
  const float t0 = knots[0], tl = knots[nk - 1];
  float xc = fminf(fmaxf(xn, t0), tl);                         // kan.py:16
  const int j = kan_search(xc, knots, nk, t0, inv_h0);
  if (j >= nb) {                                               // truncation: SURVEY.md 0.2
    r.j = -1; r.v[0] = r.v[1] = r.v[2] = r.v[3] = 0.f;
    if (DERIV) dv[0] = dv[1] = dv[2] = dv[3] = 0.f;
    return r;
  }
  const float tj = knots[j];
  const float h = knots[j + 1] - tj;
  if (!kan_locally_uniform(knots, j, h)) {
    r.j = j;
    kan_basis_general<DERIV>(xc, knots, j, r.v, dv);
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (j - m < 0) { r.v[m] = 0.f; if (DERIV) dv[m] = 0.f; }
    return r;
  }
  const float u = (xc - tj) / h;
  const float u2 = u * u, u3 = u2 * u, om = 1.f - u;
  r.j = j;
  r.v[0] = u3 * (1.f / 6.f);
  r.v[1] = (-3.f * u3 + 3.f * u2 + 3.f * u + 1.f) * (1.f / 6.f);
  r.v[2] = (3.f * u3 - 6.f * u2 + 4.f) * (1.f / 6.f);
  r.v[3] = om * om * om * (1.f / 6.f);
  if (DERIV) {
    const float ih = 1.f / h;
    dv[0] = 0.5f * u2 * ih;
    dv[1] = (-9.f * u2 + 6.f * u + 3.f) * (1.f / 6.f) * ih;
    dv[2] = (9.f * u2 - 12.f * u) * (1.f / 6.f) * ih;
    dv[3] = -0.5f * om * om * ih;
  }
#pragma unroll
  for (int m = 0; m < 4; ++m)
    if (j - m < 0) { r.v[m] = 0.f; if (DERIV) dv[m] = 0.f; }   // left edge loses terms
  return r;
}

// kan_basis's clamp and search alone, for callers that need the index inside the truncated zone too (kan_basis reports -1 for all
// of it): kan_stats.hip's occupancy counts.
__device__ __forceinline__ int kan_interval(float xn, const float* knots, int nk, float inv_h0) {
  const float t0 = knots[0], tl = knots[nk - 1];
  return kan_search(fminf(fmaxf(xn, t0), tl), knots, nk, t0, inv_h0);
}

__device__ __forceinline__ float act_apply(float z, int act) {
  if (act == ROVIT_ACT_RELU) return fmaxf(z, 0.f);
  if (act == ROVIT_ACT_SIGMOID3) return 3.f / (1.f + __expf(-z));
  return z;
}
// d(act)/dz expressed through the post-activation value y
__device__ __forceinline__ float act_grad(float g, float y, int act) {
  if (act == ROVIT_ACT_RELU) return y > 0.f ? g : 0.f;
  if (act == ROVIT_ACT_SIGMOID3) return g * y * (1.f - y * (1.f / 3.f));
  return g;
}

}  // namespace
