// Seeds of Grad-CAM++ for the severity and uncertainty outputs: the scalar per image that a target names, and its gradient with respect to
// the backbone features, d target / d features (B,192).  rovit_vit_gradcam_seeded (vit.hip) carries that gradient down to the last
// block's norm1 output and into the CAM; the class-logit seed stays in gradcam.hip (rovit_vit_gradcam).
//
// Reference being restated, with eval semantics (no dropout, whatever the Dropout modules' flags say):
//   ordinal_severity  predict()['ordinal_severity'] = sum_k k P(y = k), P from the cumulative sigmoids (models/heads.py:45-77)
//                     = (C - 1) - sum_j sigma(z_j), so d/dz_j = -sigma'(z_j)
//   mu, log_var       UncertaintyHead.forward (heads.py:91-102); log_var = clamp(pre, -10, 10), whose gradient passes where
//                     -10 <= pre <= 10 (torch.clamp's rule)
//   kan_severity      KANSeverityModule.forward (models/kan.py:138-149): autograd of the truncated spline as the head phase's backward
//                     computes it -- zero past the cutoff, tanh', and the linear branch
//
// explain_seed_kernel: ONE workgroup (4 waves) per image.
//   features -> LDS; the basis (value and derivative rows) of every KAN input; fc1 + ReLU of the ordinal / uncertainty head when a
//   target needs it; the KAN stack forward, layer by layer; the heads' output linears.  Then, for each requested target in the
//   caller's order, its value (T,B) and seed (T,B,192): heads by the transposed fc1 product of dL/d(hidden), the KAN stack top-down.
//   Only what the requested targets need runs; a target's arithmetic does not depend on which other targets are requested, so one
//   multi-target call gives the bits of the single-target calls.
// Arithmetic is fp32 (kan_device.h's basis and activations, head_phase.h's basis rows), sums in the order noted at each; no atomics,
// so every result is bit-identical from run to run.
#include "common.h"
#include "kan_device.h"
#include "head_phase.h"

namespace {

constexpr int EX_E = 192, EX_NT = 256, EX_MAX_TARGETS = 4;
constexpr int QKV = 3 * EX_E;
constexpr int WT_PER_THREAD = 16, WT_WGS = QKV * EX_E / (256 * WT_PER_THREAD);    // as gradcam.hip's seed launch
static_assert(WT_WGS * 256 * WT_PER_THREAD == QKV * EX_E, "the weight copy must tile exactly");

struct ExTargets {
  int n;
  int kind[EX_MAX_TARGETS];            // ROVIT_TARGET_* (not CLASS)
  int need_ord, need_unc, need_kan;
};

struct ExLds {
  float x[EX_E];
  float bas0[8 * EX_E], dbas0[8 * EX_E], f0[EX_E];           // layer-0 basis rows of tanh(x): value, derivative; 1 - tanh^2
  float basl[8 * HP_MAXW], fl[HP_MAXW];                       // the same for the current layer behind the first
  float knots[4][KAN_MAX_KNOTS];
  float a[4][HP_MAXW];                                        // post-activation output of every KAN layer
  float part[EX_NT];                                          // forward partial sums [slice][out]
  float gz[2][HP_MAXW];                                       // backward: gradient w.r.t. a layer's pre-activation (ping-pong)
  float ho[HP_MAX_HID], hu[HP_MAX_HID], dh[HP_MAX_HID];       // hidden of the ordinal / uncertainty head; dL/d(pre-ReLU)
  float sig[HP_MAX_CLS];                                      // sigma(z_j) of the ordinal thresholds
  float mu, lvp;                                              // mu and log_var before the clamp
};

// one KAN layer behind its basis rows: thread = (output o, input slice); terms x_i lw[o,i] + sum_k basis_k(tanh x_i) W[i,o,k] summed
// over the slice's inputs in order, the slices in order after the bias
template <int NBC>
__device__ __forceinline__ void ex_layer_fwd(const rovit_head_phase& p, ExLds& s, int l, const float* in_v, const float* bas, int tid) {
  const int in = p.kan_dims[l], out = p.kan_dims[l + 1], nb = p.kan_knots[l] - 4;
  const int S = EX_NT / out, fps = (in + S - 1) / S;
  const int sl = tid / out, o = tid - sl * out;
  const float* W = p.kan_w[l];
  const float* lw = p.kan_lw[l];
  if (sl < S) {
    const int i0 = sl * fps, i1 = min(in, i0 + fps);
    float acc = 0.f;
    for (int i = i0; i < i1; ++i) acc += fmaf(in_v[i], lw[(size_t)o * in + i], hp_dot_basis<NBC>(bas + 8 * i, W + ((size_t)i * out + o) * nb));
    s.part[sl * out + o] = acc;
  }
  __syncthreads();
  if (tid < out) {
    float z = p.kan_lb[l][tid];
    for (int q = 0; q < S; ++q) z += s.part[q * out + tid];
    s.a[l][tid] = act_apply(z, p.kan_acts[l]);
  }
  __syncthreads();
}

template <int NBC>
__global__ __launch_bounds__(EX_NT) void explain_seed_kernel(const rovit_head_phase p, const ExTargets tg, float* __restrict__ values,
                                                             float* __restrict__ seeds) {
  __shared__ __attribute__((aligned(16))) ExLds s;
  const int tid = threadIdx.x, b = blockIdx.x, B = p.batch, hid = p.hid, C = p.num_classes, L = p.kan_layers;

  if (tid < EX_E) s.x[tid] = p.features[(size_t)b * EX_E + tid];
  if (tg.need_kan)
    for (int l = 0; l < L; ++l)
      if (tid < p.kan_knots[l]) s.knots[l][tid] = p.kan_knots_p[l][tid];
  __syncthreads();

  if (tg.need_kan && tid < EX_E) {                  // the forward's basis and the backward's derivative basis of every feature
    const float xn = tanhf(s.x[tid]);
    float dv[4];
    const Basis4 bs = kan_basis<true>(xn, s.knots[0], p.kan_knots[0], 1.f / (s.knots[0][1] - s.knots[0][0]), dv);
    hp_store_basis<NBC>(s.bas0 + 8 * tid, bs.j, bs.v);
    hp_store_basis<NBC>(s.dbas0 + 8 * tid, bs.j, dv);
    s.f0[tid] = 1.f - xn * xn;                      // d tanh; the clamp is the identity on (-1, 1)
  }
  {                                                 // fc1 + ReLU of the heads a target needs: bias, then features in order
    const int R = (tg.need_ord ? hid : 0) + (tg.need_unc ? hid : 0);
    for (int r = tid; r < R; r += EX_NT) {
      const bool ord = tg.need_ord && r < hid;
      const int k = ord || !tg.need_ord ? r : r - hid;
      const float* w = (ord ? p.head_params[4] : p.head_params[8]) + (size_t)k * EX_E;
      float acc = (ord ? p.head_params[5] : p.head_params[9])[k];
      for (int d = 0; d < EX_E; ++d) acc = fmaf(w[d], s.x[d], acc);
      (ord ? s.ho : s.hu)[k] = fmaxf(acc, 0.f);
    }
  }
  __syncthreads();

  if (tg.need_kan) {
    ex_layer_fwd<NBC>(p, s, 0, s.x, s.bas0, tid);
    for (int l = 1; l < L; ++l) {
      if (tid < p.kan_dims[l]) {
        const Basis4 bs = kan_basis<false>(tanhf(s.a[l - 1][tid]), s.knots[l], p.kan_knots[l], 1.f / (s.knots[l][1] - s.knots[l][0]), nullptr);
        hp_store_basis<NBC>(s.basl + 8 * tid, bs.j, bs.v);
      }
      __syncthreads();
      ex_layer_fwd<NBC>(p, s, l, s.a[l - 1], s.basl, tid);
    }
  }
  // the heads' output linears: bias, then hidden units in order
  if (tg.need_ord && tid < C - 1) {
    const float* w = p.head_params[6] + (size_t)tid * hid;
    float z = p.head_params[7][tid];
    for (int k = 0; k < hid; ++k) z = fmaf(w[k], s.ho[k], z);
    s.sig[tid] = 1.f / (1.f + expf(-z));
  }
  if (tg.need_unc && tid >= 64 && tid < 66) {
    const int j = tid - 64;
    const float* w = p.head_params[10 + 2 * j];
    float z = p.head_params[11 + 2 * j][0];
    for (int k = 0; k < hid; ++k) z = fmaf(w[k], s.hu[k], z);
    if (j == 0) s.mu = z; else s.lvp = z;
  }
  __syncthreads();

  for (int t = 0; t < tg.n; ++t) {
    const int kind = tg.kind[t];
    float* seed = seeds + ((size_t)t * B + b) * EX_E;
    float value = 0.f;
    if (kind == ROVIT_TARGET_KAN_SEVERITY) {
      // top-down: gz = dL/d(pre-activation) of layer l; d input_i = sum_o gz[o] (W-spline' (tanh x_i) (1 - tanh^2 x_i) + lw[o,i]),
      // the outputs in order (the head phase's per-term formula)
      value = s.a[L - 1][0];
      if (tid == 0) s.gz[(L - 1) & 1][0] = act_grad(1.f, value, p.kan_acts[L - 1]);
      for (int l = L - 1; l >= 0; --l) {
        const int in = p.kan_dims[l], out = p.kan_dims[l + 1], nb = p.kan_knots[l] - 4;
        const float* bas = s.dbas0;
        const float* f = s.f0;
        __syncthreads();                            // gz of layer l complete; the layer above is done with basl / fl
        if (l > 0) {
          if (tid < in) {
            const float xn = tanhf(s.a[l - 1][tid]);
            float dv[4];
            const Basis4 bs = kan_basis<true>(xn, s.knots[l], p.kan_knots[l], 1.f / (s.knots[l][1] - s.knots[l][0]), dv);
            hp_store_basis<NBC>(s.basl + 8 * tid, bs.j, dv);
            s.fl[tid] = 1.f - xn * xn;
          }
          __syncthreads();
          bas = s.basl;
          f = s.fl;
        }
        if (tid < in) {
          const float* W = p.kan_w[l];
          const float* lw = p.kan_lw[l];
          const float* gz = s.gz[l & 1];
          float g = 0.f;
          for (int o = 0; o < out; ++o)
            g += gz[o] * fmaf(hp_dot_basis<NBC>(bas + 8 * tid, W + ((size_t)tid * out + o) * nb), f[tid], lw[(size_t)o * in + tid]);
          if (l == 0) seed[tid] = g;
          else s.gz[(l - 1) & 1][tid] = act_grad(g, s.a[l - 1][tid], p.kan_acts[l - 1]);
        }
      }
    } else {
      // dL/d(hidden) through the output linear, gated by the ReLU; then d features = W1^T dh, hidden units in order
      const bool ord = kind == ROVIT_TARGET_ORDINAL_SEVERITY;
      const float* h = ord ? s.ho : s.hu;
      if (ord) {
        // P_0 = s_0, P_k = s_k - s_{k-1}, P_{C-1} = 1 - s_{C-2}; sum_k k P_k with k in order (predict()'s expression)
        float v = 0.f;
        for (int k = 1; k < C; ++k) v = fmaf((float)k, (k < C - 1 ? s.sig[k] : 1.f) - s.sig[k - 1], v);
        value = v;
      } else {
        value = kind == ROVIT_TARGET_MU ? s.mu : fminf(fmaxf(s.lvp, -10.f), 10.f);
      }
      const bool gate = kind != ROVIT_TARGET_LOG_VAR || (s.lvp >= -10.f && s.lvp <= 10.f);
      if (tid < hid) {
        float dh = 0.f;
        if (ord) {
          for (int j = 0; j < C - 1; ++j) dh = fmaf(-s.sig[j] * (1.f - s.sig[j]), p.head_params[6][(size_t)j * hid + tid], dh);   // thresholds in order
        } else if (gate) {
          dh = p.head_params[kind == ROVIT_TARGET_MU ? 10 : 12][tid];
        }
        s.dh[tid] = h[tid] > 0.f ? dh : 0.f;
      }
      __syncthreads();
      if (tid < EX_E) {
        const float* w1 = p.head_params[ord ? 4 : 8] + tid;
        float g = 0.f;
        for (int k = 0; k < hid; ++k) g = fmaf(w1[(size_t)k * EX_E], s.dh[k], g);
        seed[tid] = g;
      }
    }
    if (tid == 0) values[(size_t)t * B + b] = value;
    __syncthreads();                                // the next target reuses dh / gz
  }
}

// wt[col][k] = bf16(Wqkv[k][col]): the same copy gradcam.hip's seed launch writes beside the class seed
__global__ __launch_bounds__(256) void explain_wt_kernel(const float* __restrict__ wqkv, bf16* __restrict__ wt) {
  const int base = (int)blockIdx.x * 256 * WT_PER_THREAD + (int)threadIdx.x;
#pragma unroll 4
  for (int e = 0; e < WT_PER_THREAD; ++e) {
    const int i = base + e * 256;
    wt[i] = (bf16)wqkv[(size_t)(i % QKV) * EX_E + i / QKV];
  }
}

}  // namespace

// (internal, common.h) the bf16 transposed copy (192, 576) of the unfolded qkv weight that gradcam.hip's g product reads
int rovit_gradcam_wt(const float* wqkv, void* wt, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(wqkv && wt, ROVIT_ERR_NULL, "gradcam_wt: null pointer");
  hipLaunchKernelGGL(explain_wt_kernel, dim3(WT_WGS), dim3(256), 0, (hipStream_t)stream, wqkv, (bf16*)wt);
  ROVIT_CHECK_LAUNCH("explain_wt_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_explain_seed(const rovit_head_phase* p, const int* kinds, int n_targets, float* values, float* seeds,
                                  rovit_stream_t stream) {
  const int rc = hp_check_params(p, "explain_seed");
  if (rc) return rc;
  ROVIT_CHECK_ARG(kinds && values && seeds, ROVIT_ERR_NULL, "explain_seed: null kinds / values / seeds");
  ROVIT_CHECK_ARG(p->embed == EX_E, ROVIT_ERR_SHAPE, "explain_seed: the features must be %d wide, got %d", EX_E, p->embed);
  ROVIT_CHECK_ARG(n_targets >= 1 && n_targets <= EX_MAX_TARGETS, ROVIT_ERR_SHAPE, "explain_seed: %d targets (1..%d)", n_targets,
                  EX_MAX_TARGETS);
  ExTargets tg{};
  tg.n = n_targets;
  for (int t = 0; t < n_targets; ++t) {
    const int k = kinds[t];
    ROVIT_CHECK_ARG(k >= ROVIT_TARGET_ORDINAL_SEVERITY && k <= ROVIT_TARGET_KAN_SEVERITY, ROVIT_ERR_SHAPE,
                    "explain_seed: target kind %d is not one of ordinal_severity (1), mu (2), log_var (3), kan_severity (4)", k);
    for (int u = 0; u < t; ++u) ROVIT_CHECK_ARG(kinds[u] != k, ROVIT_ERR_SHAPE, "explain_seed: target kind %d repeated", k);
    const int need = k == ROVIT_TARGET_ORDINAL_SEVERITY ? 2 : (k == ROVIT_TARGET_KAN_SEVERITY ? 4 : 3);
    ROVIT_CHECK_ARG(p->stage >= need, ROVIT_ERR_SHAPE, "explain_seed: target kind %d needs curriculum stage %d, the model is at %d", k, need,
                    p->stage);
    tg.kind[t] = k;
    tg.need_ord |= k == ROVIT_TARGET_ORDINAL_SEVERITY;
    tg.need_unc |= k == ROVIT_TARGET_MU || k == ROVIT_TARGET_LOG_VAR;
    tg.need_kan |= k == ROVIT_TARGET_KAN_SEVERITY;
  }
  if (tg.need_kan)
    ROVIT_CHECK_ARG(p->kan_layers >= 1 && p->kan_dims[p->kan_layers] == 1, ROVIT_ERR_SHAPE,
                    "explain_seed: kan_severity needs a KAN stack with one output (%d layers, last width %d)", p->kan_layers,
                    p->kan_layers ? p->kan_dims[p->kan_layers] : 0);
  const int nbc = tg.need_kan ? hp_nbc(p) : 7;
  if (nbc == 7) hipLaunchKernelGGL(explain_seed_kernel<7>, dim3(p->batch), dim3(EX_NT), 0, (hipStream_t)stream, *p, tg, values, seeds);
  else if (nbc == 8) hipLaunchKernelGGL(explain_seed_kernel<8>, dim3(p->batch), dim3(EX_NT), 0, (hipStream_t)stream, *p, tg, values, seeds);
  else hipLaunchKernelGGL(explain_seed_kernel<0>, dim3(p->batch), dim3(EX_NT), 0, (hipStream_t)stream, *p, tg, values, seeds);
  ROVIT_CHECK_LAUNCH("explain_seed_kernel");
  return ROVIT_OK;
}
