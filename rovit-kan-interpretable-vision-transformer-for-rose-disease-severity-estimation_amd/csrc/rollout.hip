// Attention rollout (Abnar & Zuidema 2020) folded into the forward: row 0 of  A^_1 A^_2 ... A^_depth  as a running vector.
//
// Reference being restated: ViTAttentionRollout.generate (the reference's explainability/attention_maps.py:40-105): per block the
// three heads' softmax probabilities are fused (mean / max / min over heads), the identity is added, the rows are renormalised and
// the depth matrices are multiplied; the map is row 0 of the product without the class-token entry, reshaped to 14x14, resized to
// 224x224 (cv2.resize INTER_LINEAR) and min-max normalised.
//
// Only row 0 of the product is used, so with v_0 = e_0 each block is a vector-matrix step  v <- v A^_l.  rovit_rollout_step runs
// right behind a block's attention on its saved qkv (bf16, (B*197, 576)); the 197x197 matrices live in registers and are never
// stored.  788 bytes per image leave the forward instead of 12 x 3 x 197 x 197 fp32 probabilities (5.6 MB).
//
// Step kernel: one workgroup (4 waves) = 16 query rows of one image, 13 workgroups per image (13 x 16 = 208 >= 197), so batch 1
// already spreads over 13 CUs.  Per head the K slice of the image (197 x 64 bf16, row stride 144 B: every 16-lane group of a
// ds_read_b128 hits 16 distinct 16-byte bank slots) and the workgroup's 16 query rows sit in LDS.  Each wave owns 4 query rows;
// lane l holds keys l, l+64, l+128, l+192.  Scores are fp32 FMAs on the bf16 operands, d = 0..63 in order, scaled, max-subtracted,
// __expf'd and normalised exactly as attn_probs_kernel (attention.hip) does, so the probabilities are the bits the prob taps
// return; each K read from LDS feeds the wave's 4 rows.  The heads are fused in registers, r_i = sum_j F[i,j] + 1 is a wave sum of
// the fused row, and  v_i (F[i,j] + delta_ij) / r_i  is accumulated per key.
//
// Determinism: no atomics.  The 4 waves' partial vectors are added in wave order through LDS, each workgroup writes its partial
// (B, 13, 197) slice to a scratch buffer, and a second small launch (rollout_combine_kernel) adds the 13 slices in slice order into
// v.  Every sum has a fixed order, so a rollout is bit-identical run to run at a given batch.
//
// rovit_rollout_map: one workgroup per image; bilinear 14x14 -> 224x224 with half-pixel centres and edge clamping (the arithmetic
// of F.interpolate(mode='bilinear', align_corners=False), which is what cv2.resize INTER_LINEAR does on a float image), then
// (m - min) / (max - min + 1e-8) over the image.  Two passes over the 50176 outputs (min/max, then write); no intermediate buffer.
#include "common.h"
#include "map224.h"

namespace {

constexpr int RT = 197, RH = 3, RHD = 64, RLD = 3 * RH * RHD;   // tokens, heads, head dim, qkv row length
constexpr int ROWS_WG = 16, ROWS_WAVE = 4;
constexpr int KST = RHD + 8;                                    // LDS row stride in bf16 (144 B)

__global__ __launch_bounds__(256) void rollout_step_kernel(const bf16* __restrict__ qkv, const float* __restrict__ v,
                                                           float* __restrict__ partial, int mode, int first) {
  __shared__ __attribute__((aligned(16))) bf16 ks[RT * KST];
  __shared__ __attribute__((aligned(16))) bf16 qs[ROWS_WG * KST];
  __shared__ float wpart[4][RT];
  const int split = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row0 = split * ROWS_WG;
  const bf16* base = qkv + (size_t)b * RT * RLD;

  float f[ROWS_WAVE][4];                 // fused probabilities of the wave's rows, keys lane + 64u
  for (int h = 0; h < RH; ++h) {
    if (h) __syncthreads();              // the previous head's K / Q reads are done
    for (int c = tid; c < RT * 8; c += 256) {
      const int row = c >> 3, kc = c & 7;
      *(bf16x8*)(ks + row * KST + kc * 8) = *(const bf16x8*)(base + (size_t)row * RLD + RH * RHD + h * RHD + kc * 8);
    }
    if (tid < ROWS_WG * 8) {
      const int row = tid >> 3, kc = tid & 7, qr = row0 + row;
      const bf16x8 q = *(const bf16x8*)(base + (size_t)(qr < RT ? qr : RT - 1) * RLD + h * RHD + kc * 8);
      *(bf16x8*)(qs + row * KST + kc * 8) = keep_if(q, qr < RT);
    }
    __syncthreads();
    float s[ROWS_WAVE][4];
#pragma unroll
    for (int r = 0; r < ROWS_WAVE; ++r)
#pragma unroll
      for (int u = 0; u < 4; ++u) s[r][u] = 0.f;
#pragma unroll 1                         // (fully unrolled, every LDS read is hoisted: 256 VGPRs)
    for (int kc = 0; kc < 8; ++kc) {
      bf16x8 kv[4], qv[ROWS_WAVE];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int key = lane + 64 * u;
        kv[u] = *(const bf16x8*)(ks + (key < RT ? key : RT - 1) * KST + kc * 8);
      }
#pragma unroll
      for (int r = 0; r < ROWS_WAVE; ++r) qv[r] = *(const bf16x8*)(qs + (w * ROWS_WAVE + r) * KST + kc * 8);   // broadcast
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int r = 0; r < ROWS_WAVE; ++r)
#pragma unroll
          for (int u = 0; u < 4; ++u) s[r][u] = fmaf((float)qv[r][e], (float)kv[u][e], s[r][u]);
    }
    // softmax per row, as attn_probs_kernel: scale, wave max, __expf(s - max), wave sum, multiply by the reciprocal
#pragma unroll
    for (int r = 0; r < ROWS_WAVE; ++r) {
      float mx = -INFINITY;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        s[r][u] = lane + 64 * u < RT ? s[r][u] * 0.125f : -INFINITY;
        mx = fmaxf(mx, s[r][u]);
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      float sum = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) { s[r][u] = lane + 64 * u < RT ? __expf(s[r][u] - mx) : 0.f; sum += s[r][u]; }
      sum = wave_sum64(sum);
      const float inv = 1.f / sum;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float p = s[r][u] * inv;
        if (h == 0) f[r][u] = p;
        else if (mode == 1) f[r][u] = fmaxf(f[r][u], p);
        else if (mode == 2) f[r][u] = fminf(f[r][u], p);
        else f[r][u] += p;
      }
    }
  }
  // A^[i,j] = (F[i,j] + delta_ij) / (sum_j F[i,j] + 1);  acc[j] = sum over the wave's rows i of v_i A^[i,j]
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < ROWS_WAVE; ++r) {
    const int i = row0 + w * ROWS_WAVE + r;
    if (i >= RT) break;                  // wave-uniform
    float rs = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (mode == 0) f[r][u] = f[r][u] / 3.f;
      rs += f[r][u];                     // (keys >= 197 hold 0)
    }
    const float ri = wave_sum64(rs) + 1.f;
    const float vi = first ? (i == 0 ? 1.f : 0.f) : v[(size_t)b * RT + i];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = lane + 64 * u;
      acc[u] = fmaf(vi, (f[r][u] + (j == i ? 1.f : 0.f)) / ri, acc[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (lane + 64 * u < RT) wpart[w][lane + 64 * u] = acc[u];
  __syncthreads();
  if (tid < RT) {
    const float p = ((wpart[0][tid] + wpart[1][tid]) + wpart[2][tid]) + wpart[3][tid];
    partial[((size_t)b * gridDim.x + split) * RT + tid] = p;
  }
}

__global__ __launch_bounds__(256) void rollout_combine_kernel(const float* __restrict__ partial, float* __restrict__ v, int splits) {
  const int b = blockIdx.x, j = threadIdx.x;
  if (j >= RT) return;
  const float* p = partial + (size_t)b * splits * RT + j;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += p[(size_t)k * RT];
  v[(size_t)b * RT + j] = s;
}

__global__ __launch_bounds__(256) void rollout_map_kernel(const float* __restrict__ rollout, float* __restrict__ map) {
  __shared__ float g[GRID * GRID];
  __shared__ float red[2][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < GRID * GRID) g[tid] = rollout[(size_t)b * RT + 1 + tid];
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
  const float den = mx - mn + 1e-8f;
  float* out = map + (size_t)b * MAP * MAP;
  for (int p = tid; p < MAP * MAP; p += 256) out[p] = (bilinear14(g, p / MAP, p % MAP) - mn) / den;
}

}  // namespace

// One block's rollout update (internal: vit.hip launches it behind each attention of rovit_vit_forward_rollout).
// qkv bf16 (B*197, 576); v fp32 (B,197), updated in place (first != 0: v is taken as e_0 and not read);
// partial: fp32 scratch of batch x 13 x 197 floats.
int rovit_rollout_step(const void* qkv, float* v, float* partial, int head_fusion, int batch, int first, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(qkv && v && partial, ROVIT_ERR_NULL, "rollout_step: null pointer");
  ROVIT_CHECK_ARG(batch > 0 && head_fusion >= 0 && head_fusion <= 2, ROVIT_ERR_SHAPE, "rollout_step: bad batch %d / head_fusion %d", batch,
                  head_fusion);
  constexpr int splits = (RT + ROWS_WG - 1) / ROWS_WG;
  hipLaunchKernelGGL(rollout_step_kernel, dim3(splits, batch), dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, v, partial, head_fusion,
                     first);
  ROVIT_CHECK_LAUNCH("rollout_step_kernel");
  hipLaunchKernelGGL(rollout_combine_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, partial, v, splits);
  ROVIT_CHECK_LAUNCH("rollout_combine_kernel");
  return ROVIT_OK;
}

// The reference's map from the rollout vector: attention_maps.py:96-103 (mask = rollout[0, 1:], reshape 14x14, cv2.resize to
// 224x224, (m - min) / (max - min + 1e-8)), for every image of the batch.
extern "C" int rovit_rollout_map(const float* rollout, float* map224, int batch, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(rollout && map224, ROVIT_ERR_NULL, "rollout_map: null pointer");
  ROVIT_CHECK_ARG(batch > 0, ROVIT_ERR_SHAPE, "rollout_map: bad batch %d", batch);
  hipLaunchKernelGGL(rollout_map_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, rollout, map224);
  ROVIT_CHECK_LAUNCH("rollout_map_kernel");
  return ROVIT_OK;
}
