// The nonconformity scores of split conformal prediction (conformal.hip): ONE set of device functions for the fit
// (rovit_eval_conformal) and the application (rovit_eval_conformal_apply), so calibration and test scores cannot drift apart.
// Definitions: include/rovit_hip.h, the rovit_eval_conf comment.
#pragma once
#include "common.h"
#include "philox.h"
#include "sort_device.h"

namespace conformal {

constexpr int MAXC = ROVIT_EVAL_MAX_CLASSES;

// u of one row: ((w >> 8) + 0.5) 2^-24 in two fp32 operations (the product is by a power of two: exact)
__device__ __forceinline__ float draw_u(unsigned long long seed, unsigned row) {
  const unsigned w = philox4x32_10(seed, row, 0u, ROVIT_EVAL_CONF_STREAM, 0u).x;
  return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-8f;
}

// One row's probabilities in rank order: p descending, ties by lower class index first.
struct Sorted {
  float p[MAXC];
  int idx[MAXC];
  float cum[MAXC];          // fp32 running sum in rank order, up to and including the slot
  bool nan;                 // a NaN probability: the order means nothing
};

__device__ __forceinline__ void sort_row(const float* __restrict__ row, int C, Sorted& s) {
  s.nan = false;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const float v = c < C ? row[c] : -__builtin_inff();          // the padding sinks behind every class
    s.p[c] = v;
    s.idx[c] = c;
    s.nan |= v != v;
  }
  // insertion sort with static indices (registers): an element moves left only past strictly smaller ones, hence stable
#pragma unroll
  for (int i = 1; i < MAXC; ++i) {
#pragma unroll
    for (int j = i; j >= 1; --j) {
      const bool up = s.p[j] > s.p[j - 1];
      const float pa = s.p[j - 1], pb = s.p[j];
      const int ia = s.idx[j - 1], ib = s.idx[j];
      s.p[j - 1] = up ? pb : pa;
      s.p[j] = up ? pa : pb;
      s.idx[j - 1] = up ? ib : ia;
      s.idx[j] = up ? ia : ib;
    }
  }
  float run = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    if (c < C) run += s.p[c];
    s.cum[c] = run;
  }
}

// s(c) of a class score with class c in the place of the label; 0 <= c < C
__device__ __forceinline__ float class_score(int kind, const Sorted& s, int c, float u, float lambda, int k_reg) {
  float pc = 0.f, cum = 0.f;
  int r = 0;
#pragma unroll
  for (int t = 0; t < MAXC; ++t) {
    if (s.idx[t] == c) {
      pc = s.p[t];
      cum = s.cum[t];
      r = t + 1;
    }
  }
  if (kind == ROVIT_EVAL_CONF_LAC) return (1.0f - pc) + 0.0f;
  if (s.nan) return __builtin_nanf("");
  float v = __fmaf_rn(-u, pc, cum);
  if (kind == ROVIT_EVAL_CONF_RAPS) v = __fmaf_rn(lambda, (float)max(0, r - k_reg), v);
  return v + 0.0f;
}

__device__ __forceinline__ bool is_class_kind(int kind) { return kind <= ROVIT_EVAL_CONF_RAPS; }

// the score of row i for a kind that has no per-class form; `sigma_ok` is false where _MU_SCALED has no valid sigma
__device__ __forceinline__ float row_score(const rovit_eval_conf& a, int m, int i, bool& sigma_ok) {
  sigma_ok = true;
  float v;
  switch (a.score_kind[m]) {
    case ROVIT_EVAL_CONF_KAN_ABS: v = fabsf(a.sev_true[i] - a.sev_pred[i]); break;
    case ROVIT_EVAL_CONF_MU_ABS: v = fabsf(a.sev_true[i] - a.mu[i]); break;
    case ROVIT_EVAL_CONF_MU_SCALED: {
      const float sg = a.uncertainty[i];
      sigma_ok = isfinite(sg) && sg > 0.f;
      v = fabsf(a.sev_true[i] - a.mu[i]) / sg;
      break;
    }
    default: v = a.score_column[m][i]; break;
  }
  return v + 0.0f;
}

// the order-preserving key of an fp32 value (numbers only), and back: shared with the radix sort (sort_device.h)
using ::order_key;
using ::key_bits;

}  // namespace conformal
