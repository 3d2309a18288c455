// Grad-CAM++ at blocks[-1].norm1 for a whole batch, from the last block's class-token backward (vit.hip: rovit_vit_gradcam).
//
// Reference being restated: GradCAMPlusPlus.compute (the reference's explainability/gradcam.py:34-104).  With a = the output of
// blocks[-1].norm1 (197 x 192 per image, CLS included) and g = d cls_logits[c] / d a, per image:
//   S[d] = sum_n a[n,d] g[n,d]^3,   den = 2 g^2 + S[d] (0 -> 1),   w[n] = sum_d g^2 / den * relu(g),
//   cam[n] = w[n] * sum_d a[n,d],   map = minmax(resize224(relu(cam[1:]) as 14x14))   (min-max only when max > 0).
// In eval mode the images of a batch do not interact, so one backward of sum_b cls_logits[b, c_b] gives every image its own gradient.
//
// Launches (all on the caller's stream):
//   gradcam_seed_kernel  one workgroup per image: the classification head (fc1, ReLU, fc2; no dropout) on the backbone features, the
//                        target (the caller's, or the first argmax), and d_features = W1^T (1[h > 0] * W2[c,:]) -- the seed the class-
//                        token backward starts from.  27 extra workgroups write the bf16 transposed copy of the UNFOLDED qkv weight
//                        (192 x 576) that the g product reads (the prepared images have norm1's gamma folded in).
//   [rovit_cls_tail_bwd, rovit_attention_cls_bwd: dqkv (M, 576) of the last block -- vit.hip]
//   gradcam_grad_kernel  g = dqkv . Wqkv on the matrix cores and the per-slice partial sums of S; g is kept in an fp32 scratch.
//   gradcam_cam_kernel   S from the slice partials in slice order, then w[n], sum_d a[n,d] and the relu'd cam row.
//   gradcam_map_kernel   (rovit_gradcam_map) resize + the reference's conditional min-max.
//
// g kernel: one workgroup (4 waves) = 16 token rows of one image, 13 workgroups per image (13 x 16 = 208 >= 197), so batch 1 spreads
// over 13 CUs.  Wave w owns output columns 48w .. 48w+47 (three 16x16 tiles); K = 576 in 18 steps of mfma_f32_16x16x32_bf16.  The A
// fragment (16 dqkv rows) comes straight from HBM / L2 as one 16-byte load per lane and step, the B fragments from the 221 KB bf16
// weight copy, which every workgroup streams from L2 (rows past 196 are zeroed in registers, never read past the image).
// a = xhat1 * gamma + beta is rebuilt in fp32 from the saved bf16 xhat1, as rovit_hip.taps.norm1_output does for the hook path.
//
// S[d] needs every token's g before any w[n] exists.  g is kept (fp32, 38.7 MB at batch 256) rather than recomputed in the second
// pass: DESIGN.md section 4 has the measured comparison (the developer library's knob ROVIT_KNOB_GRADCAM_RECOMPUTE builds the other one).
//
// Precision: the CAM arithmetic past g (a g^3, S, den, g^2 / den, both row sums, their product) runs in fp64.  S sums 197 terms
// of either sign and den = 2 g^2 + S can cancel, so an fp32 restatement is off by up to 1.5e-4 of the image's maximum at batch 64
// (measured); in fp64 the raw cam matches an fp64 restatement on the same fp32 taps to rounding.  ~12 fp64 divisions per lane.
//
// Determinism: no atomics.  Column sums of S: 4 rows per lane in row order, then a fixed xor butterfly over the lane groups; the 13 slice
// partials are added in slice order.  Row sums of w and sum_d a: 3 columns per lane in order, a 16-lane butterfly, the 4 waves in wave
// order.  Every result is bit-identical run to run.
#include "common.h"
#include "map224.h"

namespace {

constexpr int T = 197, D = 192, QKV = 3 * D;
constexpr int ROWS_WG = 16, SPLITS = ROVIT_GRADCAM_SPLITS;
static_assert(SPLITS * ROWS_WG >= T, "the row slices must cover the tokens");
constexpr int WT_PER_THREAD = 16, WT_WGS = QKV * D / (256 * WT_PER_THREAD);   // 27 workgroups write the transposed weight
static_assert(WT_WGS * 256 * WT_PER_THREAD == QKV * D, "the weight copy must tile exactly");

__global__ __launch_bounds__(256) void gradcam_seed_kernel(const float* __restrict__ feat, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, int hidden, int classes,
                                                           const int* __restrict__ targets, float* __restrict__ logits,
                                                           int* __restrict__ chosen, float* __restrict__ dfeat,
                                                           const float* __restrict__ wqkv, bf16* __restrict__ wt, int batch) {
  __shared__ float s_f[D], s_h[ROVIT_GRADCAM_MAX_HIDDEN], s_l[ROVIT_GRADCAM_MAX_CLASSES];
  __shared__ int s_c;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= batch) {      // wt[col][k] = bf16(Wqkv[k][col]): coalesced writes, the strided reads hit L2
    const int base = ((int)blockIdx.x - batch) * 256 * WT_PER_THREAD + tid;
#pragma unroll 4
    for (int e = 0; e < WT_PER_THREAD; ++e) {
      const int i = base + e * 256;
      wt[i] = (bf16)wqkv[(size_t)(i % QKV) * D + i / QKV];
    }
    return;
  }
  const int b = blockIdx.x;
  if (tid < D) s_f[tid] = feat[(size_t)b * D + tid];
  __syncthreads();
  for (int j = tid; j < hidden; j += 256) {            // fc1 + ReLU (dropout is off: eval semantics)
    const float* w = w1 + (size_t)j * D;
    float acc = b1[j];
    for (int k = 0; k < D; ++k) acc = fmaf(w[k], s_f[k], acc);
    s_h[j] = acc > 0.f ? acc : 0.f;
  }
  __syncthreads();
  for (int c = tid; c < classes; c += 256) {           // fc2
    const float* w = w2 + (size_t)c * hidden;
    float acc = b2[c];
    for (int j = 0; j < hidden; ++j) acc = fmaf(w[j], s_h[j], acc);
    s_l[c] = acc;
    logits[(size_t)b * classes + c] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    if (targets) {
      c = targets[b];
    } else {                                           // torch.argmax: the first maximum wins
      float best = s_l[0];
      for (int k = 1; k < classes; ++k)
        if (s_l[k] > best) { best = s_l[k]; c = k; }
    }
    s_c = c;
    if (chosen) chosen[b] = c;
  }
  __syncthreads();
  const int c = s_c;
  if (tid < D) {
    // an out-of-range target (the Python layer refuses them before launching) poisons the image instead of reading past W2
    float acc = __builtin_nanf("");
    if (c >= 0 && c < classes) {
      acc = 0.f;
      const float* w2c = w2 + (size_t)c * hidden;
      for (int j = 0; j < hidden; ++j)
        if (s_h[j] > 0.f) acc = fmaf(w1[(size_t)j * D + tid], w2c[j], acc);
    }
    dfeat[(size_t)b * D + tid] = acc;
  }
}

struct CamArgs {
  const bf16* dqkv;                    // (B*197, 576) bf16, the last block's
  const bf16* wt;                      // (192, 576) bf16: the unfolded qkv weight, transposed
  const bf16* xhat1;                   // (B*197, 192) bf16, the last block's normalised norm1 input
  const float* gamma; const float* beta;
  float* g;                            // (B*197, 192) fp32 scratch
  double* spart;                       // (B, SPLITS, 192) fp64 partial sums of S
  float* act; float* grad;             // optional (B,197,192) fp32 taps
  float* cam;                          // (B, 196) fp32
};

__device__ __forceinline__ double group4_sum_f64(double v) { v += __shfl_xor(v, 16); v += __shfl_xor(v, 32); return v; }
__device__ __forceinline__ double wave_sum16_f64(double v) {   // sum over the 16 lanes sharing l>>4
  v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
  return v;
}

// g for rows row0 .. row0+15 of one image, columns 48w .. 48w+47: acc[t][r] = g[row0 + 4 (lane >> 4) + r][48w + 16t + (lane & 15)]
__device__ __forceinline__ void g_tile(const bf16* __restrict__ dqkv, const bf16* __restrict__ wt, int row0, int w, int lane, f32x4 acc[3]) {
  const int ar = row0 + (lane & 15);
  const bf16* ap = dqkv + (size_t)(ar < T ? ar : T - 1) * QKV + 8 * (lane >> 4);
  const bf16* bp = wt + (size_t)(48 * w + (lane & 15)) * QKV + 8 * (lane >> 4);
#pragma unroll
  for (int t = 0; t < 3; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 6
  for (int kk = 0; kk < QKV / 32; ++kk) {
    const bf16x8 a = keep_if(*(const bf16x8*)(ap + 32 * kk), ar < T);
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t] = mfma16(a, *(const bf16x8*)(bp + (size_t)16 * t * QKV + 32 * kk), acc[t]);
  }
}

__global__ __launch_bounds__(256) void gradcam_grad_kernel(const CamArgs a) {
  const int split = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row0 = split * ROWS_WG;
  f32x4 acc[3];
  g_tile(a.dqkv + (size_t)b * T * QKV, a.wt, row0, w, lane, acc);
  double s[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int col = 48 * w + 16 * t + (lane & 15);
    const float ga = a.gamma[col], be = a.beta[col];
    s[t] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = row0 + 4 * (lane >> 4) + r;
      if (n < T) {
        const size_t idx = ((size_t)b * T + n) * D + col;
        const float g = acc[t][r];
        const float x = (float)a.xhat1[idx] * ga + be;
        const double gd = g;
        s[t] = fma((double)x * gd, gd * gd, s[t]);
        a.g[idx] = g;
        if (a.act) a.act[idx] = x;
        if (a.grad) a.grad[idx] = g;
      }
    }
    s[t] = group4_sum_f64(s[t]);
  }
  if (lane < 16) {
    double* sp = a.spart + ((size_t)b * SPLITS + split) * D + 48 * w + lane;
#pragma unroll
    for (int t = 0; t < 3; ++t) sp[16 * t] = s[t];
  }
}

template <bool RECOMPUTE>
__global__ __launch_bounds__(256) void gradcam_cam_kernel(const CamArgs a) {
  __shared__ double s_S[D];
  __shared__ double s_w[4][ROWS_WG], s_a[4][ROWS_WG];
  const int split = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row0 = split * ROWS_WG;
  if (tid < D) {
    const double* sp = a.spart + (size_t)b * SPLITS * D + tid;
    double S = 0.0;
    for (int k = 0; k < SPLITS; ++k) S += sp[(size_t)k * D];
    s_S[tid] = S;
  }
  f32x4 acc[3];
  if (RECOMPUTE) {
    g_tile(a.dqkv + (size_t)b * T * QKV, a.wt, row0, w, lane, acc);
  } else {
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = row0 + 4 * (lane >> 4) + r;
        acc[t][r] = n < T ? a.g[((size_t)b * T + n) * D + 48 * w + 16 * t + (lane & 15)] : 0.f;
      }
  }
  __syncthreads();
  double wr[4] = {0.0, 0.0, 0.0, 0.0}, xr[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int col = 48 * w + 16 * t + (lane & 15);
    const float ga = a.gamma[col], be = a.beta[col];
    const double S = s_S[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = row0 + 4 * (lane >> 4) + r;
      const int nc = n < T ? n : T - 1;
      const double g = acc[t][r], g2 = g * g;
      const double den0 = 2.0 * g2 + S;
      const double den = den0 != 0.0 ? den0 : 1.0;
      wr[r] += g2 / den * (g > 0.0 ? g : 0.0);
      const float x = (float)a.xhat1[((size_t)b * T + nc) * D + col] * ga + be;     // the act tap's value
      xr[r] += x;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    wr[r] = wave_sum16_f64(wr[r]);
    xr[r] = wave_sum16_f64(xr[r]);
  }
  if ((lane & 15) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s_w[w][4 * (lane >> 4) + r] = wr[r];
      s_a[w][4 * (lane >> 4) + r] = xr[r];
    }
  }
  __syncthreads();
  if (tid < ROWS_WG) {
    const int n = row0 + tid;
    if (n >= 1 && n < T) {
      const double wn = ((s_w[0][tid] + s_w[1][tid]) + s_w[2][tid]) + s_w[3][tid];
      const double xn = ((s_a[0][tid] + s_a[1][tid]) + s_a[2][tid]) + s_a[3][tid];
      const double c = wn * xn;
      a.cam[(size_t)b * (T - 1) + n - 1] = c > 0.0 ? (float)c : 0.f;
    }
  }
}

// resize to 224x224, then (m - min) / (max - min) when max > 0, else the map as it is (gradcam.py:93-101)
__global__ __launch_bounds__(256) void gradcam_map_kernel(const float* __restrict__ cam, float* __restrict__ map) {
  __shared__ float g[GRID * GRID];
  __shared__ float red[2][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < GRID * GRID) g[tid] = cam[(size_t)b * GRID * GRID + tid];
  __syncthreads();
  float mn = INFINITY, mx = -INFINITY;
  for (int p = tid; p < MAP * MAP; p += 256) {
    const float m = bilinear14(g, p / MAP, p % MAP);
    mn = fminf(mn, m);
    mx = fmaxf(mx, m);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
  if (lane == 0) { red[0][w] = mn; red[1][w] = mx; }
  __syncthreads();
  mn = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
  mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  // no epsilon, as the reference: an all-equal positive map divides 0 by 0 and comes out NaN there and here
  const bool norm = mx > 0.f;
  const float den = mx - mn;
  float* out = map + (size_t)b * MAP * MAP;
  for (int p = tid; p < MAP * MAP; p += 256) {
    const float m = bilinear14(g, p / MAP, p % MAP);
    out[p] = norm ? (m - mn) / den : m;
  }
}

}  // namespace

// (internal, common.h) the head seed of rovit_vit_gradcam and the bf16 transposed copy of the unfolded qkv weight
int rovit_gradcam_seed(const float* feat, const float* w1, const float* b1, const float* w2, const float* b2, int hidden, int classes,
                       const int* targets, float* logits, int* chosen, float* dfeat, const float* wqkv, void* wt, int batch,
                       rovit_stream_t stream) {
  ROVIT_CHECK_ARG(feat && w1 && b1 && w2 && b2 && logits && dfeat && wqkv && wt, ROVIT_ERR_NULL, "gradcam_seed: null pointer");
  ROVIT_CHECK_ARG(batch > 0 && hidden > 0 && hidden <= ROVIT_GRADCAM_MAX_HIDDEN && classes > 0 && classes <= ROVIT_GRADCAM_MAX_CLASSES,
                  ROVIT_ERR_SHAPE, "gradcam_seed: bad batch %d / hidden %d / classes %d", batch, hidden, classes);
  hipLaunchKernelGGL(gradcam_seed_kernel, dim3(batch + WT_WGS), dim3(256), 0, (hipStream_t)stream, feat, w1, b1, w2, b2, hidden, classes,
                     targets, logits, chosen, dfeat, wqkv, (bf16*)wt, batch);
  ROVIT_CHECK_LAUNCH("gradcam_seed_kernel");
  return ROVIT_OK;
}

// (internal, common.h) g, S and the raw cam of every image from the last block's dqkv
int rovit_gradcam_cam(const void* dqkv, const void* wt, const void* xhat1, const float* gamma, const float* beta, float* g, double* spart,
                      float* act, float* grad, float* cam, int batch, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(dqkv && wt && xhat1 && gamma && beta && g && spart && cam, ROVIT_ERR_NULL, "gradcam_cam: null pointer");
  ROVIT_CHECK_ARG(batch > 0, ROVIT_ERR_SHAPE, "gradcam_cam: bad batch %d", batch);
  ROVIT_CHECK_ARG(rovit_aligned16(dqkv) && rovit_aligned16(wt), ROVIT_ERR_ALIGN, "gradcam_cam: dqkv / wt must be 16-byte aligned");
  const CamArgs a{(const bf16*)dqkv, (const bf16*)wt, (const bf16*)xhat1, gamma, beta, g, spart, act, grad, cam};
  hipLaunchKernelGGL(gradcam_grad_kernel, dim3(SPLITS, batch), dim3(256), 0, (hipStream_t)stream, a);
  ROVIT_CHECK_LAUNCH("gradcam_grad_kernel");
#ifdef ROVIT_DEV
  if (ROVIT_KNOB(ROVIT_KNOB_GRADCAM_RECOMPUTE, 0)) {
    hipLaunchKernelGGL(gradcam_cam_kernel<true>, dim3(SPLITS, batch), dim3(256), 0, (hipStream_t)stream, a);
    ROVIT_CHECK_LAUNCH("gradcam_cam_kernel<recompute>");
    return ROVIT_OK;
  }
#endif
  hipLaunchKernelGGL(gradcam_cam_kernel<false>, dim3(SPLITS, batch), dim3(256), 0, (hipStream_t)stream, a);
  ROVIT_CHECK_LAUNCH("gradcam_cam_kernel");
  return ROVIT_OK;
}

// The reference's map from the raw cam (gradcam.py:89-101): relu'd 14x14 grid, cv2.resize to 224x224, min-max when max > 0.
extern "C" int rovit_gradcam_map(const float* cam, float* map224, int batch, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(cam && map224, ROVIT_ERR_NULL, "gradcam_map: null pointer");
  ROVIT_CHECK_ARG(batch > 0, ROVIT_ERR_SHAPE, "gradcam_map: bad batch %d", batch);
  hipLaunchKernelGGL(gradcam_map_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, cam, map224);
  ROVIT_CHECK_LAUNCH("gradcam_map_kernel");
  return ROVIT_OK;
}
