// Per-sample device routines and host checks shared by the head-phase kernels (head_phase.hip) and the explanation seed (explain.hip):
// the limits of a rovit_head_phase descriptor, the basis rows of one KAN input in LDS and their dot product with a W[i, o, :] row.
#pragma once
#include "common.h"
#include "kan_device.h"

namespace {

constexpr int HP_MAXW = 64;           // widest KAN layer behind the input
constexpr int HP_MAX_EMBED = 768, HP_MAX_HID = 256, HP_MAX_CLS = 8;

// basis row of one input in LDS, 8 floats.  NBC = 7 / 8 (num_basis known at compile time; 7 is the reference's default, num_knots 5):
// the DENSE row d[k], so that a W[i, o, :] row is a plain dot product of whole-row loads (two instructions that do not depend on the
// interval index; the 28-byte rows of num_basis 7 are only dword-aligned: dword-aligned dwordx4 / dwordx3 loads, which gfx950 under
// ROCm executes in unaligned-access mode and hipcc emits for align-4 vector types).  NBC = 0 (any other num_basis): slots 0..3 the
// four non-zero values in the order of the four CONSECUTIVE weights they meet, slot 4 the first weight's index: one dword-aligned
// 16-byte load per (input, output) pair (four separate gathers of one dword each took the forward from 40 to 82 us at num_knots 32).
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x3u __attribute__((ext_vector_type(3), aligned(4)));
template <int NBC>
__device__ __forceinline__ void hp_store_basis(float* dst, int j, const float* v) {
  if (NBC) {
    float d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = k == j ? v[0] : (k == j - 1 ? v[1] : (k == j - 2 ? v[2] : (k == j - 3 ? v[3] : 0.f)));
    *(float4*)dst = make_float4(d[0], d[1], d[2], d[3]);
    *(float4*)(dst + 4) = make_float4(d[4], d[5], d[6], d[7]);
  } else {
    // the four live values ALIGNED to the four consecutive weights w[j0 .. j0 + 3], j0 = max(j, 3) - 3: u[k] pairs with w[j0 + k]
    // (j >= 3: u = v[3], v[2], v[1], v[0]; at the left edge, j < 3, the window starts at 0 and the missing terms are zeros)
    const int j0 = (j > 3 ? j : 3) - 3, sft = j - j0;          // sft = 3, or j at the left edge (-1: no live term, v is all zero)
    float u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int m = sft - k;
      u[k] = m == 0 ? v[0] : (m == 1 ? v[1] : (m == 2 ? v[2] : (m == 3 ? v[3] : 0.f)));
    }
    *(float4*)dst = make_float4(u[0], u[1], u[2], u[3]);
    dst[4] = __int_as_float(j0);
  }
}
// sum_k basis[k] W[k] for the (nb,) row at w
template <int NBC>
__device__ __forceinline__ float hp_dot_basis(const float* bas, const float* __restrict__ w) {
  if (NBC == 8) {
    const float4 w0 = *(const float4*)w, w1 = *(const float4*)(w + 4);
    const float4 d0 = *(const float4*)bas, d1 = *(const float4*)(bas + 4);
    float t = d0.x * w0.x;
    t = fmaf(d0.y, w0.y, t); t = fmaf(d0.z, w0.z, t); t = fmaf(d0.w, w0.w, t);
    t = fmaf(d1.x, w1.x, t); t = fmaf(d1.y, w1.y, t); t = fmaf(d1.z, w1.z, t); t = fmaf(d1.w, w1.w, t);
    return t;
  } else if (NBC == 7) {
    const f32x4u w0 = *(const f32x4u*)w;
    const f32x3u w1 = *(const f32x3u*)(w + 4);
    const float4 d0 = *(const float4*)bas, d1 = *(const float4*)(bas + 4);
    float t = d0.x * w0.x;
    t = fmaf(d0.y, w0.y, t); t = fmaf(d0.z, w0.z, t); t = fmaf(d0.w, w0.w, t);
    t = fmaf(d1.x, w1.x, t); t = fmaf(d1.y, w1.y, t); t = fmaf(d1.z, w1.z, t);
    return t;
  } else {
    const float4 u = *(const float4*)bas;
    const f32x4u wv = *(const f32x4u*)(w + __float_as_int(bas[4]));      // ONE dword-aligned 16-byte load of the four live weights
    float t = u.x * wv.x;
    t = fmaf(u.y, wv.y, t); t = fmaf(u.z, wv.z, t); t = fmaf(u.w, wv.w, t);
    return t;
  }
}

// every shape and parameter pointer of a descriptor (not the forward's output buffers)
int hp_check_params(const rovit_head_phase* p, const char* who) {
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->batch > 0 && p->embed >= 4 && p->embed <= HP_MAX_EMBED && p->embed % 4 == 0, ROVIT_ERR_SHAPE,
                  "%s: batch %d / embed %d (embed: multiple of 4, <= %d)", who, p->batch, p->embed, HP_MAX_EMBED);
  ROVIT_CHECK_ARG(p->hid >= 4 && p->hid <= HP_MAX_HID && p->hid % 4 == 0, ROVIT_ERR_SHAPE, "%s: hidden width %d (multiple of 4, <= %d)", who,
                  p->hid, HP_MAX_HID);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= HP_MAX_CLS, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who, p->num_classes, HP_MAX_CLS);
  ROVIT_CHECK_ARG(p->stage >= 1 && p->stage <= 4, ROVIT_ERR_SHAPE, "%s: curriculum stage %d not in 1..4", who, p->stage);
  ROVIT_CHECK_ARG(p->kan_layers >= 0 && p->kan_layers <= 4, ROVIT_ERR_SHAPE, "%s: %d KAN layers (0..4)", who, p->kan_layers);
  ROVIT_CHECK_ARG(p->drop_p >= 0.f && p->drop_p < 1.f, ROVIT_ERR_SHAPE, "%s: dropout probability %g", who, (double)p->drop_p);
  ROVIT_CHECK_ARG(p->features && rovit_aligned16(p->features), ROVIT_ERR_NULL, "%s: features (16-byte aligned) missing", who);
  const int nheads = p->stage >= 3 ? 3 : (p->stage >= 2 ? 2 : 1);
  for (int h = 0; h < nheads; ++h) {
    const int n = h == 2 ? 6 : 4;
    for (int q = 0; q < n; ++q)
      ROVIT_CHECK_ARG(p->head_params[4 * h + q] && rovit_aligned16(p->head_params[4 * h + q]), ROVIT_ERR_ALIGN,
                      "%s: head parameter %d missing or not 16-byte aligned", who, 4 * h + q);
  }
  if (p->kan_layers) {
    ROVIT_CHECK_ARG(p->kan_dims[0] == p->embed, ROVIT_ERR_SHAPE, "%s: the KAN stack's input width %d is not the feature width %d", who,
                    p->kan_dims[0], p->embed);
    for (int l = 0; l < p->kan_layers; ++l) {
      ROVIT_CHECK_ARG(p->kan_dims[l + 1] >= 1 && p->kan_dims[l + 1] <= HP_MAXW, ROVIT_ERR_SHAPE, "%s: KAN layer %d is %d wide (1..%d)", who, l,
                      p->kan_dims[l + 1], HP_MAXW);
      ROVIT_CHECK_ARG(p->kan_knots[l] >= 8 && p->kan_knots[l] <= KAN_MAX_KNOTS, ROVIT_ERR_SHAPE, "%s: KAN layer %d has %d knots (8..%d)", who, l,
                      p->kan_knots[l], KAN_MAX_KNOTS);
      ROVIT_CHECK_ARG(p->kan_w[l] && p->kan_knots_p[l] && p->kan_lw[l] && p->kan_lb[l], ROVIT_ERR_NULL,
                      "%s: KAN layer %d: null pointer", who, l);
      ROVIT_CHECK_ARG(rovit_aligned16(p->kan_w[l]) && rovit_aligned16(p->kan_lw[l]), ROVIT_ERR_ALIGN, "%s: KAN layer %d weights not 16-byte aligned", who, l);
    }
  }
  return ROVIT_OK;
}
int hp_check(const rovit_head_phase* p, const char* who) {
  const int rc = hp_check_params(p, who);
  if (rc) return rc;
  ROVIT_CHECK_ARG(p->hidden, ROVIT_ERR_NULL, "%s: features (16-byte aligned) / hidden missing", who);
  for (int l = 0; l < p->kan_layers; ++l) ROVIT_CHECK_ARG(p->kan_out[l], ROVIT_ERR_NULL, "%s: KAN layer %d: null pointer", who, l);
  return ROVIT_OK;
}

// 7 / 8 when every layer has that num_basis (the dense-row kernels), else 0
int hp_nbc(const rovit_head_phase* p) {
  int nb = p->kan_layers ? p->kan_knots[0] - 4 : 7;
  for (int l = 1; l < p->kan_layers; ++l)
    if (p->kan_knots[l] - 4 != nb) nb = 0;
  return (nb == 7 || nb == 8) ? nb : 0;
}

}  // namespace
