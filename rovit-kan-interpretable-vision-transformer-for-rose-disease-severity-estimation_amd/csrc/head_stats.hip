// Per-head attention statistics folded into the forward: entropy, mean attention distance, class-token mass, self mass, row maximum
// and 3x3 locality of every (image, block, head), the class token's own attention row, and optionally four values per query row.
//
// Definitions (rovit_hip/head_stats.py restates them in numpy fp64; include/rovit_hip.h lists the summary's eight entries).  P is the
// 197 x 197 softmax of one (image, block, head); token 0 is the class token, patch t >= 1 sits at (r, c) = divmod(t - 1, 14);
// dist(i, j) = 16 sqrt((r_i - r_j)^2 + (c_i - c_j)^2) pixels; 0 ln 0 = 0.  Per query row i:
//   H_i = -sum_j P_ij ln P_ij          D_i = sum_{j>=1} P_ij dist(i,j) / sum_{j>=1} P_ij  (i >= 1; 0 for i = 0 and when the patches' mass is 0)
//   C_i = P_i0                         M_i = max_j P_ij
//
// Step kernel: the launch shape of rollout_step_kernel (rollout.hip) -- one workgroup (4 waves) = 16 query rows of one image, 13
// workgroups per image, K slice of the head (197 x 64 bf16, row stride 144 B) and the 16 query rows in LDS, each wave owns 4 rows, lane l
// holds keys l, l+64, l+128, l+192 -- and its arithmetic for the scores and the softmax, copied and not shared: fp32 FMAs on the bf16
// operands, d = 0..63 in order, x 0.125, wave max, __expf, wave sum, reciprocal.  The probabilities are the bits rovit_attention_probs
// writes.  They stay in registers; per head every row gives five wave reductions (entropy, distance sum, patch mass, locality, max) and
// two lane reads (P_i0, P_ii).  The logarithm is logf, not __logf: the entropy is compared with an fp64 oracle at 9.4e-5 ln 197.
//
// Why 13 workgroups per image and a combine launch, not one workgroup per (image, head) without one: a workgroup per (image, head) would
// walk 197 rows with 4 waves (13 passes over the same K tile) and batch 1 would occupy 3 CUs of 256; K in LDS is 28 KB either way, so the
// LDS bounds neither shape at 160 KB per CU (5 workgroups of this kernel fit: 31.5 KB each), and the per-image K reload (13 x 28 KB from L2)
// is small beside the 64 FMAs per (query, key) pair.  The 13-way split keeps batch 1 on 13 CUs and costs one 24-float partial per workgroup.
// Registers: 108 VGPRs, 106 SGPRs, no scratch (-O3, kernel-resource-usage remark) -- 4 waves per SIMD, so 4 workgroups per CU; the
// registers, not the LDS, set that limit.
//
// Determinism, and the order of every sum (tests/test_gpu_head_stats.py reproduces it in fp32 from per_token, bit for bit): no atomics.
// A wave adds its 4 rows' values in row order; the 4 waves' partials go through LDS and are added ((w0 + w1) + w2) + w3; each workgroup
// writes 3 x 8 partials to scratch; head_stats_combine_kernel adds the 13 slices in slice order and multiplies by the constant 1/197 or
// 1/196.  Padding rows 197..207 of the last slice add nothing (the row loop stops at 197).  H_0 and P_00 (entries 4 and 5) are not sums: the
// one wave that owns row 0 assigns them, every other wave and slice holds 0 there, so they pass through the same additions unchanged (x + 0
// is exact) and are multiplied by 1.
//
// Finalise kernel: one thread per (group, column) of the recorded rows, group 0 = every row, group 1 + c = rows labelled c; the thread walks
// the rows in storage order twice in fp64 (mean, then sum of squared deviations).  The order depends on the rows' positions alone, so the
// block is bit-identical however the rows arrived in the buffer.  The launch has (classes + 1) x (R + Q) threads (36 720 at depth 12 with 4
// classes), each a serial chain of 2n fp64 additions that re-reads the n labels in both passes: sized for the data sets this model sees,
// n up to a few 10^4 images, and not measured beyond the tests' n = 300; for n of 10^5 and more the rows would want a split with a
// fixed-order second stage.
#include "common.h"

namespace {

constexpr int RT = 197, RH = 3, RHD = 64, RLD = 3 * RH * RHD;   // tokens, heads, head dim, qkv row length
constexpr int ROWS_WG = 16, ROWS_WAVE = 4;
constexpr int KST = RHD + 8;                                    // LDS row stride in bf16 (144 B)
constexpr int NS = 8, NPATCH = RT - 1, GRID14 = 14;
constexpr int SPLITS = (RT + ROWS_WG - 1) / ROWS_WG;            // 13

__global__ __launch_bounds__(256) void head_stats_step_kernel(const bf16* __restrict__ qkv, float* __restrict__ partial,
                                                              float* __restrict__ cls_attention, float* __restrict__ per_token, int block,
                                                              int depth) {
  __shared__ __attribute__((aligned(16))) bf16 ks[RT * KST];
  __shared__ __attribute__((aligned(16))) bf16 qs[ROWS_WG * KST];
  __shared__ float wpart[RH][4][NS];
  const int split = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row0 = split * ROWS_WG;
  const bf16* base = qkv + (size_t)b * RT * RLD;

  // grid cell of the lane's four keys (key 0, the class token, and keys >= 197 take no part in the distance or the locality)
  int kr[4], kc_[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int t = lane + 64 * u - 1;
    kr[u] = t >= 0 ? t / GRID14 : 0;
    kc_[u] = t >= 0 ? t % GRID14 : 0;
  }

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
#pragma unroll 1
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
    float acc[NS];                       // the wave's sums over its rows, the same value in every lane
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.f;
#pragma unroll
    for (int r = 0; r < ROWS_WAVE; ++r) {
      const int i = row0 + w * ROWS_WAVE + r;
      if (i >= RT) break;                // wave-uniform: the padding rows of the last slice
      // softmax of the row, as attn_probs_kernel: scale, wave max, __expf(s - max), wave sum, multiply by the reciprocal
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
      const int ir = i >= 1 ? (i - 1) / GRID14 : 0, ic = i >= 1 ? (i - 1) % GRID14 : 0;
      float ent = 0.f, dsum = 0.f, pmass = 0.f, loc = 0.f, pmax = 0.f, pself = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = lane + 64 * u;
        const float p = s[r][u] * inv;   // (keys >= 197 hold 0)
        s[r][u] = p;
        ent -= p > 0.f ? p * logf(p) : 0.f;
        pmax = fmaxf(pmax, p);
        if (j == i) pself = p;
        if (j >= 1 && j < RT) {
          const int dr = kr[u] - ir, dc = kc_[u] - ic;
          pmass += p;
          dsum = fmaf(p, 16.f * sqrtf((float)(dr * dr + dc * dc)), dsum);
          if (dr >= -1 && dr <= 1 && dc >= -1 && dc <= 1) loc += p;
        }
      }
      ent = wave_sum64(ent);
      dsum = wave_sum64(dsum);
      pmass = wave_sum64(pmass);
      loc = wave_sum64(loc);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, o));
      pself = __shfl(pself, i & 63);     // key i lives in lane i mod 64 (its slot i / 64 set pself there and nowhere else)
      const float pcls = __shfl(s[r][0], 0);
      const float dist = (i >= 1 && pmass > 0.f) ? dsum / pmass : 0.f;
      acc[0] += ent;
      acc[3] += pself;
      acc[6] += pmax;
      if (i >= 1) {
        acc[1] += dist;
        acc[2] += pcls;
        acc[7] += loc;
      } else {
        acc[4] = ent;
        acc[5] = pcls;
        float* ca = cls_attention + (((size_t)b * depth + block) * RH + h) * NPATCH;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = lane + 64 * u;
          if (j >= 1 && j < RT) ca[j - 1] = s[r][u];
        }
      }
      if (per_token && lane == 0) {
        f32x4 v;
        v[0] = ent; v[1] = dist; v[2] = pcls; v[3] = pmax;
        *(f32x4*)(per_token + ((((size_t)b * depth + block) * RH + h) * RT + i) * 4) = v;
      }
    }
    if (lane < NS) {
      float a = acc[0];
#pragma unroll
      for (int k = 1; k < NS; ++k) a = lane == k ? acc[k] : a;
      wpart[h][w][lane] = a;
    }
  }
  __syncthreads();
  if (tid < RH * NS) {
    const int h = tid / NS, k = tid % NS;
    partial[((size_t)b * SPLITS + split) * (RH * NS) + tid] = ((wpart[h][0][k] + wpart[h][1][k]) + wpart[h][2][k]) + wpart[h][3][k];
  }
}

__global__ __launch_bounds__(64) void head_stats_combine_kernel(const float* __restrict__ partial, float* __restrict__ summary, int block,
                                                               int depth) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (t >= RH * NS) return;
  const float* p = partial + (size_t)b * SPLITS * (RH * NS) + t;
  float s = 0.f;
  for (int k = 0; k < SPLITS; ++k) s += p[(size_t)k * (RH * NS)];
  const int k = t % NS;
  const float scale = (k == 4 || k == 5) ? 1.f : (k == 0 || k == 3 || k == 6) ? 1.f / 197.f : 1.f / 196.f;
  summary[((size_t)b * depth + block) * (RH * NS) + t] = s * scale;
}

// out: (groups) x [count, mean[R], var[R], cls_mean[Q]] doubles.  One thread per (group, column of the R + Q).
__global__ __launch_bounds__(256) void head_stats_finalize_kernel(const float* __restrict__ summary, const float* __restrict__ cls_attention,
                                                                  const int* __restrict__ labels, double* __restrict__ out, int n, int R, int Q,
                                                                  int groups) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int cols = R + Q;
  if (idx >= (long long)groups * cols) return;
  const int g = (int)(idx / cols), col = (int)(idx % cols);
  if (g > 0 && !labels) return;          // (no labels: the entry point asks for one group)
  const float* x = col < R ? summary + col : cls_attention + (col - R);
  const size_t ld = col < R ? R : Q;
  double sum = 0.0;
  long long cnt = 0;
  for (int i = 0; i < n; ++i) {
    if (g > 0 && labels[i] != g - 1) continue;
    sum += (double)x[(size_t)i * ld];
    ++cnt;
  }
  const double mean = cnt > 0 ? sum / (double)cnt : 0.0;
  double* o = out + (size_t)g * (1 + 2 * (size_t)R + Q);
  if (col == 0) o[0] = (double)cnt;
  if (col >= R) {
    o[1 + 2 * (size_t)R + (col - R)] = mean;
    return;
  }
  double ss = 0.0;
  for (int i = 0; i < n; ++i) {
    if (g > 0 && labels[i] != g - 1) continue;
    const double d = (double)x[(size_t)i * ld] - mean;
    ss += d * d;
  }
  o[1 + col] = mean;
  o[1 + R + col] = cnt > 1 ? ss / (double)(cnt - 1) : 0.0;
}

}  // namespace

extern "C" size_t rovit_head_stats_block_words(int depth, int heads, int classes) {
  if (depth < 1 || heads < 1 || classes < 0) return 0;
  const size_t R = (size_t)depth * heads * NS, Q = (size_t)depth * heads * NPATCH;
  return ((size_t)classes + 1) * (1 + 2 * R + Q);
}

extern "C" int rovit_attention_head_stats_step(const void* qkv, float* summary, float* cls_attention, float* per_token, float* partial,
                                               int batch, int block, int depth, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(qkv && summary && cls_attention && partial, ROVIT_ERR_NULL, "attention_head_stats_step: null pointer");
  ROVIT_CHECK_ARG(batch > 0 && batch <= 65535 && depth > 0 && block >= 0 && block < depth, ROVIT_ERR_SHAPE,
                  "attention_head_stats_step: bad batch %d / block %d of depth %d", batch, block, depth);
  ROVIT_CHECK_ARG(rovit_aligned16(qkv) && (!per_token || rovit_aligned16(per_token)), ROVIT_ERR_ALIGN,
                  "attention_head_stats_step: qkv and per_token must be 16-byte aligned");
  hipLaunchKernelGGL(head_stats_step_kernel, dim3(SPLITS, batch), dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, partial,
                     cls_attention, per_token, block, depth);
  ROVIT_CHECK_LAUNCH("head_stats_step_kernel");
  hipLaunchKernelGGL(head_stats_combine_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, partial, summary, block, depth);
  ROVIT_CHECK_LAUNCH("head_stats_combine_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_head_stats_finalize(const float* summary, const float* cls_attention, const int* labels, double* block, int n,
                                         int depth, int heads, int classes, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(summary && cls_attention && block, ROVIT_ERR_NULL, "head_stats_finalize: null pointer");
  ROVIT_CHECK_ARG(n > 0 && depth > 0 && depth <= 64 && heads > 0 && heads <= 64 && classes >= 0 && classes <= 4096, ROVIT_ERR_SHAPE,
                  "head_stats_finalize: bad n %d / depth %d / heads %d / classes %d", n, depth, heads, classes);
  ROVIT_CHECK_ARG(labels || classes == 0, ROVIT_ERR_NULL, "head_stats_finalize: %d classes but no labels", classes);
  const int R = depth * heads * NS, Q = depth * heads * NPATCH, groups = classes + 1;
  const long long threads = (long long)groups * (R + Q);
  hipLaunchKernelGGL(head_stats_finalize_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, summary,
                     cls_attention, labels, block, n, R, Q, groups);
  ROVIT_CHECK_LAUNCH("head_stats_finalize_kernel");
  return ROVIT_OK;
}
