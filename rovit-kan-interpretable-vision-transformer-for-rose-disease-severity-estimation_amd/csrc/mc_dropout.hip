// Monte-Carlo dropout over the three heads in ONE launch: the epistemic uncertainty the reference gets by running its model T times with
// the nn.Dropout modules in training mode (the enable_dropout() interface of the reference's experiments/baselines.py:48-52 over the
// heads' Dropout(0.3), models/heads.py:14,35,87).
//
// The backbone has no dropout (DeiT-Tiny: drop_rate, attn_drop and drop_path are 0), so its features -- and every head's relu(fc1(x)) --
// are the same in every sample.  Only the dropout mask and the small output linears behind it change.  ONE workgroup owns ONE image:
//   (A) features row -> LDS; the output linears of the active heads -> LDS (read T times below)
//   (B) relu(fc1(x)) of every active head ONCE, with the dense-row arithmetic of head_phase_fwd_kernel step (C) (4 lanes per row,
//       16-byte loads, the same sum order), kept in LDS
//   (C) wave w takes the samples t = w, w + NW, ...: lanes cover hid and draw the masks (Philox4x32-10 of philox.h, key = seed, counter
//       (b * hid + k, t, offset lo, offset hi), words x / y / z -> heads 0 / 1 / 2; kept and scaled as head_phase_fwd_kernel does, so
//       sample 0 is the training head phase's draw); the masked hidden rows go to the wave's LDS slice; 16 lanes per output row with the
//       head phase's step (D) arithmetic (models/heads.py:17-22, 38-43, 91-102 with the +-10 log_var clamp of :100)
//   (D) lanes 0..19 of the wave turn the sample's logits into per-sample quantities (probabilities from the log-softmax, their entropy, the
//       cumulative-link probabilities of OrdinalHead.probabilities_from_logits, heads.py:51-54, mu, exp(log_var)) and fold them into
//       fp64 Welford accumulators
//   (E) the waves' accumulators meet in LDS and are merged (Chan et al.) in wave order; one pass writes the per-image statistics.
// Every sum has a fixed order and no atomics are used: reruns are bit-identical, and an image's statistics depend only on (its features,
// its index b, seed, offset).
#include "common.h"
#include "philox.h"

namespace {

constexpr int MC_NT = 512, MC_NW = MC_NT / ROVIT_WAVE;
constexpr int MC_MAX_EMBED = 768, MC_MAX_HID = 256, MC_MAX_CLS = 8, MC_MAX_SAMPLES = 4096;
constexpr int MC_MAX_ROWS = 2 * MC_MAX_CLS + 1;   // C class logits + C - 1 thresholds + mu + log_var
// Welford slots of a sample (lane = slot): [0, 8) softmax probability of class c; [8, 16) ordinal probability of level c;
// 16 entropy of the sample's softmax; 17 ordinal severity sum_c c * p_ord_c; 18 mu; 19 exp(log_var)
constexpr int MC_SLOTS = 20, MC_S_ENT = 16, MC_S_SEV = 17, MC_S_MU = 18, MC_S_ALEA = 19;

__device__ __forceinline__ int mc_nheads(int stage) { return stage >= 3 ? 3 : (stage >= 2 ? 2 : 1); }

// output row r of the active heads -> (head, row of that head's weight, weight, bias)
__device__ __forceinline__ void mc_out_row(const rovit_head_mc& p, int r, int& h, const float*& w, const float*& bias) {
  const int C = p.num_classes;
  if (r < C) { h = 0; w = p.head_params[2] + (size_t)r * p.hid; bias = p.head_params[3] + r; }
  else if (r < 2 * C - 1) { h = 1; w = p.head_params[6] + (size_t)(r - C) * p.hid; bias = p.head_params[7] + (r - C); }
  else if (r == 2 * C - 1) { h = 2; w = p.head_params[10]; bias = p.head_params[11]; }
  else { h = 2; w = p.head_params[12]; bias = p.head_params[13]; }
}

struct Welford { double n, mean, m2; };
__device__ __forceinline__ void welford_add(Welford& a, double v) {
  a.n += 1.0;
  const double d = v - a.mean;
  a.mean += d / a.n;
  a.m2 += d * (v - a.mean);
}
__device__ __forceinline__ void welford_merge(Welford& a, const Welford& b) {       // Chan, Golub, LeVeque (1979)
  if (b.n == 0.0) return;
  if (a.n == 0.0) { a = b; return; }
  const double n = a.n + b.n, d = b.mean - a.mean;
  a.mean += d * (b.n / n);
  a.m2 += b.m2 + d * d * (a.n * b.n / n);
  a.n = n;
}

__global__ __launch_bounds__(MC_NT) void head_mc_fwd_kernel(const rovit_head_mc p) {
  __shared__ __attribute__((aligned(16))) float s_x[MC_MAX_EMBED];
  __shared__ __attribute__((aligned(16))) float s_h[3 * MC_MAX_HID];                  // relu(fc1(x)) of the active heads
  __shared__ __attribute__((aligned(16))) float s_w2[MC_MAX_ROWS * MC_MAX_HID];       // output linears, row r at r * hid
  __shared__ __attribute__((aligned(16))) float s_hm[MC_NW][3 * MC_MAX_HID];          // per wave: the current sample's masked rows
  __shared__ float s_out[MC_NW][MC_MAX_ROWS];                                          // per wave: the current sample's outputs
  __shared__ Welford s_acc[MC_NW][MC_SLOTS];
  __shared__ float s_mean[MC_SLOTS], s_var[MC_SLOTS];
  __shared__ double s_pbar[MC_MAX_CLS];                                                // fp64 mean class probabilities

  const int tid = threadIdx.x, lane = tid & (ROVIT_WAVE - 1), w = tid / ROVIT_WAVE, b = blockIdx.x;
  const int E = p.embed, hid = p.hid, C = p.num_classes, B = p.batch, T = p.num_samples;
  const int nheads = mc_nheads(p.stage);
  const int R2 = C + (nheads >= 2 ? C - 1 : 0) + (nheads >= 3 ? 2 : 0);

  // (A)
  for (int i = tid; i < E; i += MC_NT) s_x[i] = p.features[(size_t)b * E + i];
  for (int i = tid; i < R2 * hid; i += MC_NT) {
    const int r = i / hid, k = i - r * hid;
    int h; const float* wr; const float* br;
    mc_out_row(p, r, h, wr, br);
    s_w2[i] = wr[k];
  }
  __syncthreads();
  // (B) the dense rows of the heads' fc1, four lanes per row (head_phase_fwd_kernel step (C), same order of every sum)
  {
    const int R = nheads * hid, E4 = E / 4;
    for (int item = tid; item < R * 4; item += MC_NT) {
      const int part = item & 3, r = item >> 2, h = r / hid, k = r - h * hid;
      const float4* wrow = (const float4*)(p.head_params[4 * h] + (size_t)k * E);
      float acc = 0.f;
#pragma unroll 6
      for (int q = part; q < E4; q += 4) {
        const float4 wv = wrow[q], xv = ((const float4*)s_x)[q];
        acc = fmaf(wv.x, xv.x, acc); acc = fmaf(wv.y, xv.y, acc); acc = fmaf(wv.z, xv.z, acc); acc = fmaf(wv.w, xv.w, acc);
      }
      acc += __shfl_xor(acc, 1);
      acc += __shfl_xor(acc, 2);
      if (part == 0) s_h[r] = fmaxf(acc + p.head_params[4 * h + 1][k], 0.f);          // Linear -> ReLU (heads.py:18-19)
    }
  }
  __syncthreads();

  // (C) + (D): the samples, NW at a time (a uniform trip count: every wave reaches every barrier)
  const float drop_p = p.drop_p;
  const float keep = 1.f - drop_p, inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  Welford acc = {0.0, 0.0, 0.0};
  const int H4 = hid / 4;
  for (int t0 = 0; t0 < T; t0 += MC_NW) {
    const int t = t0 + w;
    const bool live = t < T;
    if (live) {
      for (int k = lane; k < hid; k += ROVIT_WAVE) {
        float v0 = s_h[k], v1 = nheads >= 2 ? s_h[hid + k] : 0.f, v2 = nheads >= 3 ? s_h[2 * hid + k] : 0.f;
        if (drop_p > 0.f) {                                                             // -> Dropout (heads.py:20)
          const U4 rr = philox4x32_10(p.seed, (unsigned)(b * hid + k), (unsigned)t, (unsigned)p.offset, (unsigned)(p.offset >> 32));
          v0 = (float)(rr.x >> 8) * (1.f / 16777216.f) < keep ? v0 * inv_keep : 0.f;
          v1 = (float)(rr.y >> 8) * (1.f / 16777216.f) < keep ? v1 * inv_keep : 0.f;
          v2 = (float)(rr.z >> 8) * (1.f / 16777216.f) < keep ? v2 * inv_keep : 0.f;
        }
        s_hm[w][k] = v0;
        if (nheads >= 2) s_hm[w][hid + k] = v1;
        if (nheads >= 3) s_hm[w][2 * hid + k] = v2;
      }
    }
    __syncthreads();
    if (live) {
      // the output linears, 16 lanes per row (head_phase_fwd_kernel step (D)): four rows per pass of the wave
      for (int r0 = 0; r0 < R2; r0 += 4) {
        const int r = r0 + (lane >> 4), part = lane & 15;
        const bool row = r < R2;
        int h = 0; const float* wr = nullptr; const float* br = nullptr;
        if (row) mc_out_row(p, r, h, wr, br);
        float a = 0.f;
        if (row) {
          const float4* wv = (const float4*)(s_w2 + (size_t)r * hid);
          const float4* hv = (const float4*)(&s_hm[w][h * hid]);
          for (int q = part; q < H4; q += 16) {
            const float4 x4 = wv[q], c4 = hv[q];
            a = fmaf(x4.x, c4.x, a); a = fmaf(x4.y, c4.y, a); a = fmaf(x4.z, c4.z, a); a = fmaf(x4.w, c4.w, a);
          }
        }
        a = wave_sum16(a);
        if (row && part == 0) {
          a += *br;
          if (r == 2 * C) a = fminf(fmaxf(a, -10.f), 10.f);                                 // heads.py:100
          s_out[w][r] = a;
          const size_t tb = (size_t)t * B + b;
          if (h == 0) { if (p.s_cls) p.s_cls[tb * C + r] = a; }
          else if (h == 1) { if (p.s_ord) p.s_ord[tb * (C - 1) + (r - C)] = a; }
          else if (r == 2 * C - 1) { if (p.s_mu) p.s_mu[tb] = a; }
          else if (p.s_lv) p.s_lv[tb] = a;
        }
      }
    }
    __syncthreads();
    if (live && lane < MC_SLOTS) {
      const float* o = s_out[w];
      double v = 0.0;
      bool use = false;
      if (lane < 8 || lane == MC_S_ENT) {                         // log-softmax of the class logits
        float mx = o[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, o[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(o[c] - mx);
        const float lse = mx + logf(se);
        if (lane < C) { v = expf(o[lane] - lse); use = true; }
        else if (lane == MC_S_ENT) {
          // the entropy of exactly the fp32 probabilities the class lanes fold in, in fp64 -- the function (E) applies to their mean,
          // so that identical samples (p = 0) give a mutual information of exactly 0
          double hs = 0.0;
          for (int c = 0; c < C; ++c) {
            const double pc = (double)expf(o[c] - lse);
            hs -= pc > 0.0 ? pc * log(pc) : 0.0;                  // 0 log 0 = 0
          }
          v = hs; use = true;
        }
      } else if (nheads >= 2 && ((lane >= 8 && lane < 8 + C) || lane == MC_S_SEV)) {
        // cumulative-link probabilities (heads.py:51-54): [s_0, s_1 - s_0, ..., 1 - s_{C-2}], s = sigmoid(thresholds)
        const float* th = o + C;
        auto sig = [](float z) { return 1.f / (1.f + expf(-z)); };
        auto pord = [&](int c) {
          if (c == 0) return sig(th[0]);
          if (c == C - 1) return 1.f - sig(th[C - 2]);
          return sig(th[c]) - sig(th[c - 1]);
        };
        if (lane < 8 + C) v = pord(lane - 8);
        else {
          float s = 0.f;
          for (int c = 0; c < C; ++c) s += pord(c) * (float)c;
          v = s;
        }
        use = true;
      } else if (nheads >= 3 && lane == MC_S_MU) {
        v = o[2 * C - 1]; use = true;
      } else if (nheads >= 3 && lane == MC_S_ALEA) {
        v = expf(o[2 * C]); use = true;
      }
      if (use) welford_add(acc, v);
    }
  }
  // (E) merge the waves' accumulators in wave order
  if (lane < MC_SLOTS) s_acc[w][lane] = acc;
  __syncthreads();
  Welford tot = {0.0, 0.0, 0.0};
  double var = 0.0;
  if (tid < MC_SLOTS) {
    for (int v = 0; v < MC_NW; ++v) welford_merge(tot, s_acc[v][tid]);
    var = tot.n > 0.0 ? tot.m2 / tot.n : 0.0;                      // over the T samples, divided by T
    if (var < 0.0) var = 0.0;
    s_mean[tid] = (float)tot.mean;
    s_var[tid] = (float)var;
    if (tid < MC_MAX_CLS) s_pbar[tid] = tot.mean;
  }
  __syncthreads();
  if (tid < C) {
    p.class_probs[(size_t)b * C + tid] = (float)tot.mean;
    p.class_probs_std[(size_t)b * C + tid] = (float)sqrt(var);
  } else if (tid >= 8 && tid < 8 + C) {
    if (nheads >= 2) p.ord_probs[(size_t)b * C + (tid - 8)] = (float)tot.mean;
  } else if (tid == MC_S_ENT) {
    double hp = 0.0;
    for (int c = 0; c < C; ++c) {
      const double pc = s_pbar[c];
      hp -= pc > 0.0 ? pc * log(pc) : 0.0;
    }
    const double mi = hp - tot.mean;
    p.pred_entropy[b] = (float)hp;
    p.exp_entropy[b] = (float)tot.mean;
    p.mutual_info[b] = (float)(mi > 0.0 ? mi : 0.0);
  } else if (tid == MC_S_SEV) {
    if (nheads >= 2) {
      double s = 0.0;
      for (int c = 0; c < C; ++c) s += (double)s_mean[8 + c] * c;
      p.ord_severity[b] = (float)s;
      p.ord_severity_std[b] = (float)sqrt(var);
    }
  } else if (tid == MC_S_MU) {
    if (nheads >= 3) { p.unc_mu[b] = (float)tot.mean; p.epistemic_var[b] = (float)var; }
  } else if (tid == MC_S_ALEA) {
    if (nheads >= 3) p.aleatoric_var[b] = (float)tot.mean;
  }
  __syncthreads();
  // uncertainty_std = sqrt(aleatoric + epistemic) of the two fp32 values just written
  if (tid == 0 && nheads >= 3) p.unc_std[b] = sqrtf(s_mean[MC_S_ALEA] + s_var[MC_S_MU]);
}

}  // namespace

extern "C" int rovit_head_mc_fwd(const rovit_head_mc* p, rovit_stream_t stream) {
  const char* who = "head_mc_fwd";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->batch > 0 && p->embed >= 4 && p->embed <= MC_MAX_EMBED && p->embed % 4 == 0, ROVIT_ERR_SHAPE,
                  "%s: batch %d / embed %d (batch >= 1; embed: multiple of 4, <= %d)", who, p->batch, p->embed, MC_MAX_EMBED);
  ROVIT_CHECK_ARG(p->hid >= 4 && p->hid <= MC_MAX_HID && p->hid % 4 == 0, ROVIT_ERR_SHAPE, "%s: hidden width %d (multiple of 4, <= %d)", who,
                  p->hid, MC_MAX_HID);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= MC_MAX_CLS, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who, p->num_classes,
                  MC_MAX_CLS);
  ROVIT_CHECK_ARG(p->stage >= 1 && p->stage <= 4, ROVIT_ERR_SHAPE, "%s: curriculum stage %d not in 1..4", who, p->stage);
  ROVIT_CHECK_ARG(p->num_samples >= 1 && p->num_samples <= MC_MAX_SAMPLES, ROVIT_ERR_SHAPE, "%s: %d samples (1..%d)", who, p->num_samples,
                  MC_MAX_SAMPLES);
  ROVIT_CHECK_ARG(p->drop_p >= 0.f && p->drop_p < 1.f, ROVIT_ERR_SHAPE, "%s: dropout probability %g (0 <= p < 1)", who, (double)p->drop_p);
  ROVIT_CHECK_ARG(p->features && rovit_aligned16(p->features), ROVIT_ERR_NULL, "%s: features missing or not 16-byte aligned", who);
  const int nheads = p->stage >= 3 ? 3 : (p->stage >= 2 ? 2 : 1);
  for (int h = 0; h < nheads; ++h) {
    const int n = h == 2 ? 6 : 4;
    for (int q = 0; q < n; ++q)
      ROVIT_CHECK_ARG(p->head_params[4 * h + q] && rovit_aligned16(p->head_params[4 * h + q]), ROVIT_ERR_ALIGN,
                      "%s: head parameter %d missing or not 16-byte aligned", who, 4 * h + q);
  }
  ROVIT_CHECK_ARG(p->class_probs && p->class_probs_std && p->pred_entropy && p->exp_entropy && p->mutual_info, ROVIT_ERR_NULL,
                  "%s: a classification statistic output is missing", who);
  ROVIT_CHECK_ARG(p->stage < 2 || (p->ord_probs && p->ord_severity && p->ord_severity_std), ROVIT_ERR_NULL,
                  "%s: an ordinal statistic output is missing at stage %d", who, p->stage);
  ROVIT_CHECK_ARG(p->stage < 3 || (p->unc_mu && p->epistemic_var && p->aleatoric_var && p->unc_std), ROVIT_ERR_NULL,
                  "%s: an uncertainty statistic output is missing at stage %d", who, p->stage);
  ROVIT_CHECK_ARG((p->s_ord == nullptr || p->stage >= 2) && ((p->s_mu == nullptr && p->s_lv == nullptr) || p->stage >= 3), ROVIT_ERR_SHAPE,
                  "%s: per-sample outputs of a head that stage %d does not run", who, p->stage);
  hipLaunchKernelGGL(head_mc_fwd_kernel, dim3(p->batch), dim3(MC_NT), 0, (hipStream_t)stream, *p);
  ROVIT_CHECK_LAUNCH("head_mc_fwd_kernel");
  return ROVIT_OK;
}
