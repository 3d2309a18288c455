// Gradient-weighted attention relevance (Chefer, Gur & Wolf, ICCV 2021: avg_heads + apply_self_attention_rules) folded into the
// backbone's dgrad chain: row 0 of  R_L = (I + A_L) ... (I + A_1),  A_l = mean_h relu(G_{l,h} * P_{l,h}),  G = d target / d P.
//
// Only row 0 of R_L is used, so with u = e_0 each block is a vector step  u <- u + u A_l  taken in BACKWARD order (l = L .. 1): the
// order in which rovit_vit_backward_relevance (vit.hip) visits the blocks.  No 197x197 matrix is stored.
//
// Per (image, head): P = exp2(S scale log2e - lse2) with S = Q K^T and the lse2 the training forward saved (no +3 offset: these are the
// probabilities themselves, not attention.hip's pre-scaled ones), and G = dP = dO_h V_h^T, dO the gradient with respect to the
// attention output (the proj input, step A3 of the backward).
//
// Step kernel: one workgroup (4 waves) = one (image, head).  K and V of the head sit in LDS as 208 zero-padded rows (attention.hip's
// 160-byte row stride); each wave walks 16-row query tiles w, w + 4, ... with its Q and dO row fragments read straight from global
// memory.  Both products are v_mfma_f32_16x16x32_bf16 with the QUERY on the accumulator rows and the key on the lane (A = Q / dO rows,
// B = K / V rows: every operand is a row read), so a lane holds four query rows of one key and the weighted sum over the queries,
// w_h[j] = sum_i u_i relu(P_ij dP_ij), is four FMAs per key tile in registers, then one lane-group sum and one sum over the waves.
//
// first != 0 (the last block): the training forward ran only the class token's query there (rovit_attention_cls_fwd) and the backward
// wrote only the class-token rows of dO, so lse2 and dO are valid on row 0 only -- the other rows hold whatever the recycled workspace
// held, NaN included.  u = e_0 is not read, only query row 0 is weighted, and row 0 is the only row of Q, dO and lse2 that is READ: the
// other rows of the tile are zero fragments and zero statistics, never stale bytes multiplied by zero.
//
// Determinism: no atomics.  Per key the sums run in a fixed order (query tiles of a wave in order, the four rows of a lane group in
// order, the xor-16 / xor-32 lane-group sum, the waves in order), each workgroup writes its head's partial to the scratch (B, 3, 197),
// and a second small launch adds  u[j] += (w_0[j] + w_1[j] + w_2[j]) / 3  per image.  A step is bit-identical run to run.
#include "common.h"

namespace {

constexpr int RT = 197, RH = 3, RHD = 64, RLD = 3 * RH * RHD, OLD = RH * RHD;   // tokens, heads, head dim, qkv / dO row lengths
constexpr int NT = 13, TPAD = 16 * NT;      // 16-row tiles: 208 >= 197
constexpr int KST = RHD + 16;               // LDS row stride in bf16 (160 B, as attention.hip's AST)
constexpr int NWR = 4;                      // waves per workgroup
constexpr float LOG2E = 1.4426950408889634f;
constexpr size_t REL_LDS = (size_t)2 * TPAD * KST * sizeof(bf16) + (size_t)(2 + NWR) * TPAD * sizeof(float);

__device__ __forceinline__ bf16x8 frag(const bf16* tile, int row, int ks, int lg) {
  return *(const bf16x8*)(tile + row * KST + ks * 32 + lg * 8);
}

template <bool FIRST>
__global__ __launch_bounds__(NWR * 64) void relevance_step_kernel(const bf16* __restrict__ qkv, const float* __restrict__ lse2,
                                                                const bf16* __restrict__ dout, const float* __restrict__ u,
                                                                float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) bf16 lds[];
  bf16* Ks = lds;
  bf16* Vs = Ks + TPAD * KST;
  float* s_lse = (float*)(Vs + TPAD * KST);    // [TPAD]  lse2 of the query rows (0 on rows that are not read)
  float* s_u = s_lse + TPAD;                   // [TPAD]  u of the query rows (0 on padded rows)
  float* s_w = s_u + TPAD;                     // [NWR][TPAD]  per-wave partials
  const int bh = blockIdx.x, b = bh / RH, h = bh - b * RH;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lg = lane >> 4;
  const bf16* qbase = qkv + (size_t)b * RT * RLD + h * RHD;
  const bf16* gbase = dout + (size_t)b * RT * OLD + h * RHD;
  // K / V rows [0, 197) of the head, rows 197..207 zero (clamped load + select: no read past the image's last row)
#pragma unroll
  for (int i = 0; i < (TPAD * 8 + NWR * 64 - 1) / (NWR * 64); ++i) {
    const int c = tid + i * NWR * 64;
    if (c < TPAD * 8) {
      const int row = c >> 3, kc = c & 7, rc = row < RT ? row : RT - 1;
      const bf16* src = qbase + (size_t)rc * RLD + kc * 8;
      const bf16x8 k = *(const bf16x8*)(src + RH * RHD), v = *(const bf16x8*)(src + 2 * RH * RHD);
      *(bf16x8*)(Ks + row * KST + kc * 8) = keep_if(k, row < RT);
      *(bf16x8*)(Vs + row * KST + kc * 8) = keep_if(v, row < RT);
    }
  }
  if (tid < TPAD) {
    const float* lrow = lse2 + ((size_t)b * RH + h) * RT;
    if (FIRST) {                               // row 0 only: u = e_0, the other rows' lse2 is never read
      s_lse[tid] = tid == 0 ? lrow[0] : 0.f;
      s_u[tid] = tid == 0 ? 1.f : 0.f;
    } else {
      s_lse[tid] = tid < RT ? lrow[tid] : 0.f;
      s_u[tid] = tid < RT ? u[(size_t)b * RT + tid] : 0.f;
    }
  }
  __syncthreads();
  const float c2 = 0.125f * LOG2E;             // softmax scale head_dim^-1/2 = 1/8
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  float acc[NT];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) acc[kt] = 0.f;
#pragma unroll 1
  for (int qt = w; qt < (FIRST ? 1 : NT); qt += NWR) {
    const int q0 = 16 * qt, qr = q0 + l15;
    // FIRST: every lane reads row 0 and all but the row-0 lanes keep zeros; otherwise padded rows read the last row and keep zeros
    const bool keep = FIRST ? l15 == 0 : qr < RT;
    const int qc = FIRST ? 0 : (qr < RT ? qr : RT - 1);
    bf16x8 qf[2], gf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[ks] = keep_if(*(const bf16x8*)(qbase + (size_t)qc * RLD + ks * 32 + lg * 8), keep);
      gf[ks] = keep_if(*(const bf16x8*)(gbase + (size_t)qc * OLD + ks * 32 + lg * 8), keep);
    }
    const float4 l4 = *(const float4*)(s_lse + q0 + 4 * lg), u4 = *(const float4*)(s_u + q0 + 4 * lg);
    const float lr[4] = {l4.x, l4.y, l4.z, l4.w}, ur[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      const int kr = 16 * kt + l15;
      // rows = queries q0 + 4 lg + r, column = key kr
      const f32x4 s = mfma16(qf[1], frag(Ks, kr, 1, lg), mfma16(qf[0], frag(Ks, kr, 0, lg), zero4));
      const f32x4 dp = mfma16(gf[1], frag(Vs, kr, 1, lg), mfma16(gf[0], frag(Vs, kr, 0, lg), zero4));
      float a = acc[kt];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -lr[r]));
        const float x = p * dp[r];
        a = fmaf(ur[r], x < 0.f ? 0.f : x, a);            // relu that keeps NaN, as torch.clamp(min=0) (fmaxf(NaN, 0) = 0 would hide it)
      }
      // padded keys: zero K / V rows give p = exp2(-lse2), which is Inf for lse2 < -128; their lanes are dropped, not multiplied by 0
      acc[kt] = (16 * kt + 16 <= RT || kr < RT) ? a : 0.f;
      // one key tile's fragments in flight at a time: unfenced, hipcc hoists the LDS reads of all 13 tiles (256 VGPRs, one wave per SIMD)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    const float a = group4_sum(acc[kt]);
    if (lg == 0) s_w[w * TPAD + 16 * kt + l15] = a;
  }
  __syncthreads();
  if (tid < RT) {
    float t = s_w[tid];
#pragma unroll
    for (int k = 1; k < NWR; ++k) t += s_w[k * TPAD + tid];
    part[((size_t)b * RH + h) * RT + tid] = t;
  }
}

// u[b, j] = (first ? delta_0j : u[b, j]) + (w_0[j] + w_1[j] + w_2[j]) / 3
__global__ __launch_bounds__(256) void relevance_combine_kernel(const float* __restrict__ part, float* __restrict__ u, int first) {
  const int b = blockIdx.x, j = threadIdx.x;
  if (j >= RT) return;
  const float* p = part + (size_t)b * RH * RT + j;
  const float add = ((p[0] + p[RT]) + p[2 * RT]) / 3.f;
  float* dst = u + (size_t)b * RT + j;
  *dst = (first ? (j == 0 ? 1.f : 0.f) : *dst) + add;
}

}  // namespace

// One block's relevance update (include/rovit_hip.h): u fp32 (B,197) <- u + u A, A = mean over the 3 heads of relu(P * (dO_h V_h^T)).
extern "C" int rovit_attention_relevance_step(const void* qkv, const float* lse2, const void* dout, float* u, float* scratch, int batch,
                                              int first, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(qkv && lse2 && dout && u && scratch, ROVIT_ERR_NULL, "attention_relevance_step: null pointer");
  ROVIT_CHECK_ARG(batch > 0, ROVIT_ERR_SHAPE, "attention_relevance_step: bad batch %d", batch);
  ROVIT_CHECK_ARG(rovit_aligned16(qkv) && rovit_aligned16(dout), ROVIT_ERR_ALIGN,
                  "attention_relevance_step: qkv / dout must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  if (first) {
    ROVIT_CHECK_ARG(rovit_set_max_lds((const void*)relevance_step_kernel<true>, REL_LDS), ROVIT_ERR_LAUNCH,
                    "attention_relevance_step: cannot raise the LDS limit");
    hipLaunchKernelGGL(relevance_step_kernel<true>, dim3(batch * RH), dim3(NWR * 64), REL_LDS, st, (const bf16*)qkv, lse2,
                       (const bf16*)dout, u, scratch);
  } else {
    ROVIT_CHECK_ARG(rovit_set_max_lds((const void*)relevance_step_kernel<false>, REL_LDS), ROVIT_ERR_LAUNCH,
                    "attention_relevance_step: cannot raise the LDS limit");
    hipLaunchKernelGGL(relevance_step_kernel<false>, dim3(batch * RH), dim3(NWR * 64), REL_LDS, st, (const bf16*)qkv, lse2,
                       (const bf16*)dout, u, scratch);
  }
  ROVIT_CHECK_LAUNCH("relevance_step_kernel");
  hipLaunchKernelGGL(relevance_combine_kernel, dim3(batch), dim3(256), 0, st, scratch, u, first ? 1 : 0);
  ROVIT_CHECK_LAUNCH("relevance_combine_kernel");
  return ROVIT_OK;
}
