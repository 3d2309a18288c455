// Per-row arithmetic and block reduction of the fused joint multi-task loss, shared by joint_loss_kernel (loss.hip) and
// joint_loss_mixed_kernel (train_epoch.hip).  One statement of the formulas: the two kernels cannot drift apart, and the unmixed
// instantiation is the same instruction sequence in both, which is what makes rovit_joint_loss_mixed without a second label column
// bit-identical to rovit_joint_loss.
//
// Reference being restated: training/losses.py
//   FocalLoss.forward          :15-38   alpha_t (1 - p_t)^gamma * CE, mean over the batch
//   OrdinalBCELoss.forward     :48-72   BCE-with-logits against (target > k), mean over thresholds then batch
//   UncertaintyLoss.forward    :80-101  0.5 ((y - mu)^2 exp(-s) + s), mean
//   KANRegressionLoss.forward  :109-114 MSE
//   JointLoss.forward          :139-181 total = cls + lambda*ord (stage>=2) + mu*unc (stage>=3) + nu*kan (stage>=4)
#pragma once
#include "common.h"

namespace joint_loss {

constexpr int MAXC = 16;

struct LossArgs {
  const float* cls; const float* ord; const float* mu; const float* lv; const float* kan;
  const long long* cls_t; const void* sev_t; int sev_i64; const float* alpha;
  float* d_cls; float* d_ord; float* d_mu; float* d_lv; float* d_kan;
  float* out;      // [5]: cls, ord, unc, kan, total
  int B, C;
  float lambda_ord, mu_unc, nu_kan, gamma;
};

__device__ __forceinline__ float block_sum(float v, float* s_red) {
  v = wave_sum64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// log-softmax of one logit as (z - shift) - rest, with the row's (shift, rest) from softmax_shift().  One statement, used for log p_t of
// both label columns and for every p_j.
__device__ __forceinline__ float log_softmax(float z, float shift, float rest) { return (z - shift) - rest; }

// (shift, rest) of a row whose largest logit is zmax and whose log(sum_j exp(z_j - zmax)) is lgse.
//   |zmax| >= DIRECT_BELOW: (zmax, lgse), log p_j = (z_j - zmax) - lgse.  The common shift of the logits leaves with the first subtraction,
//     which is exact to an ulp of the difference.  zmax + lgse would be rounded at the size of zmax, and z_j minus it would carry
//     ulp(zmax) / 2 into every log-probability of the row: 3e-5 for logits around 1000, three times the gradient bound of the tests.
//   |zmax| <  DIRECT_BELOW: (zmax + lgse, 0), log p_j = z_j - lse.  There |lse| < 4 + log(16) < 8, so the sum is rounded by at most
//     2^-22 = 2.4e-7: no more than the subtraction z_j - zmax of the other form loses at a gap of 8, and a fortieth of the bound.  These
//     are the floating-point operations this row has always had, and keeping them for such logits keeps a training run reproducible bit
//     for bit across the change: the bf16 backward re-rounds even a one-ulp change of the loss gradients to bf16 noise (5e-4 rms of the
//     parameter gradients after one step), and AdamW carries that on.
constexpr float DIRECT_BELOW = 4.f;
__device__ __forceinline__ void softmax_shift(float zmax, float lgse, float& shift, float& rest) {
  const bool direct = fabsf(zmax) < DIRECT_BELOW;
  shift = direct ? zmax + lgse : zmax;
  rest = direct ? 0.f : lgse;
}

// Focal term of one row for one label (losses.py:15-38): val = alpha (1 - p_t)^gamma (-log p_t) and the factor `coef` of
// d/dz_j = alpha [gamma p_t (1-p_t)^(gamma-1) log p_t - (1-p_t)^gamma] (delta_jt - p_j) / B.  log p_t is log_softmax(z[t], shift, rest).
__device__ __forceinline__ void focal_term(const LossArgs& a, const float* z, float shift, float rest, int t, float invB, float& val, float& coef) {
  const float logpt = log_softmax(z[t], shift, rest);
  const float pt = __expf(logpt);
  const float al = a.alpha ? a.alpha[t] : 1.f;
  const float om = 1.f - pt;
  const float fg = __powf(fmaxf(om, 0.f), a.gamma);                // (1 - p_t)^gamma
  val = al * fg * (-logpt);
  const float fgm1 = a.gamma == 0.f ? 0.f : a.gamma * __powf(fmaxf(om, 1e-30f), a.gamma - 1.f);
  coef = al * (fgm1 * pt * logpt - fg) * invB;
}

// One batch row: adds the row's four loss terms to the thread's accumulators and writes the row's gradients of the TOTAL loss.
// MIXED: the focal term and its gradient are lam f(t_a) + (1 - lam) f(t_b) (CutMix / MixUp, trainer.py:104-111); the log-softmax is
// computed once, and the three label-free terms once.  WANT_CORRECT: returns 1 when the row's first-maximum argmax of the logits (a NaN
// counts as the maximum, as in torch.max) equals class label a (trainer.py:151-153), else 0.
template <bool MIXED, bool WANT_CORRECT>
__device__ __forceinline__ int row(const LossArgs& a, const long long* cls_t_b, float lam, int b, float invB, float& l_cls, float& l_ord,
                                   float& l_unc, float& l_kan) {
  // an out-of-range class label would index z[] / alpha[] out of bounds: clamp it and poison the losses with NaN so
  // that the caller sees it (torch's cross_entropy raises a device assert in that case)
  const long long t_raw = a.cls_t[b];
  const bool t_ok = t_raw >= 0 && t_raw < a.C;
  const int t = t_ok ? (int)t_raw : 0;
  if (!t_ok) l_cls = __builtin_nanf("");
  int tb = 0;
  if (MIXED) {
    const long long tb_raw = cls_t_b[b];
    const bool tb_ok = tb_raw >= 0 && tb_raw < a.C;
    tb = tb_ok ? (int)tb_raw : 0;
    if (!tb_ok) l_cls = __builtin_nanf("");
  }
  // severity as float, like the reference's .float() casts (:89-90, :110-111); int64 labels are converted here, not by a copy launch
  const float y = a.sev_i64 ? (float)((const long long*)a.sev_t)[b] : ((const float*)a.sev_t)[b];
  // ---- focal cross-entropy (losses.py:15-38) ----
  float z[MAXC];
  float zmax = -INFINITY;
  for (int j = 0; j < a.C; ++j) { z[j] = a.cls[(size_t)b * a.C + j]; zmax = fmaxf(zmax, z[j]); }
  float se = 0.f;
  for (int j = 0; j < a.C; ++j) se += __expf(z[j] - zmax);
  float shift, rest;
  softmax_shift(zmax, __logf(se), shift, rest);
  float val, coef;
  focal_term(a, z, shift, rest, t, invB, val, coef);
  if (MIXED) {
    float val_b, coef_b;
    focal_term(a, z, shift, rest, tb, invB, val_b, coef_b);
    const float oml = 1.f - lam;
    l_cls += lam * val + oml * val_b;
    for (int j = 0; j < a.C; ++j) {
      const float pj = __expf(log_softmax(z[j], shift, rest));
      a.d_cls[(size_t)b * a.C + j] = lam * (coef * ((j == t ? 1.f : 0.f) - pj)) + oml * (coef_b * ((j == tb ? 1.f : 0.f) - pj));
    }
  } else {
    l_cls += val;
    for (int j = 0; j < a.C; ++j) {
      const float pj = __expf(log_softmax(z[j], shift, rest));
      a.d_cls[(size_t)b * a.C + j] = coef * ((j == t ? 1.f : 0.f) - pj);
    }
  }
  // ---- ordinal BCE (losses.py:48-72) ----
  if (a.ord) {
    const int K1 = a.C - 1;
    const float w = a.lambda_ord * invB / K1;
    float acc = 0.f;
    for (int k = 0; k < K1; ++k) {
      const float x = a.ord[(size_t)b * K1 + k];
      const float yt = y > (float)k ? 1.f : 0.f;                  // (targets > k).float(), losses.py:55-56
      acc += fmaxf(x, 0.f) - x * yt + __logf(1.f + __expf(-fabsf(x)));      // stable BCE-with-logits
      a.d_ord[(size_t)b * K1 + k] = w * (1.f / (1.f + __expf(-x)) - yt);
    }
    l_ord += acc / K1;
  }
  // ---- heteroscedastic regression (losses.py:80-101) ----
  if (a.mu) {
    const float m = a.mu[b], s = a.lv[b];
    const float prec = __expf(-s), r = y - m;
    l_unc += 0.5f * (r * r * prec + s);
    a.d_mu[b] = -a.mu_unc * invB * r * prec;
    a.d_lv[b] = a.mu_unc * invB * 0.5f * (1.f - r * r * prec);
  }
  // ---- KAN severity regression (losses.py:109-114) ----
  if (a.kan) {
    const float r = a.kan[b] - y;
    l_kan += r * r;
    a.d_kan[b] = a.nu_kan * invB * 2.f * r;
  }
  if (!WANT_CORRECT) return 0;
  int best = 0;
  float bestv = z[0];
  for (int j = 1; j < a.C; ++j)
    if (z[j] > bestv || (z[j] != z[j] && bestv == bestv)) { best = j; bestv = z[j]; }
  return (long long)best == t_raw ? 1 : 0;
}

// The batch means of the four terms and the weighted total, on every thread: r = [cls, ord, unc, kan, total]
__device__ __forceinline__ void reduce(const LossArgs& a, float invB, float l_cls, float l_ord, float l_unc, float l_kan, float* s_red, float* r) {
  const float s_cls = block_sum(l_cls, s_red) * invB;
  const float s_ord = block_sum(l_ord, s_red) * invB;
  const float s_unc = block_sum(l_unc, s_red) * invB;
  const float s_kan = block_sum(l_kan, s_red) * invB;
  r[0] = s_cls; r[1] = s_ord; r[2] = s_unc; r[3] = s_kan;
  r[4] = s_cls + (a.ord ? a.lambda_ord * s_ord : 0.f) + (a.mu ? a.mu_unc * s_unc : 0.f) + (a.kan ? a.nu_kan * s_kan : 0.f);
}

}  // namespace joint_loss
