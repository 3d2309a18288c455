// Gradient of the patch embedding with respect to its input pixels: the transpose of rovit_patch_embed_fwd (gemm.hip).
//
//   d_images[b, c, 16 py + ky, 16 px + kx]  (+)=  scale * sum_{s < copies} sum_n  dY[(s B_out + b) 197 + 1 + 14 py + px][n] W[n][c 256 + ky 16 + kx]
//
// dY: the bf16 token rows the backbone's dgrad chain leaves for the patch embedding (its class-token rows carry no pixel gradient and are
// not read); W: the prepared bf16 (192, 768) patch weight, read as the forward reads it.  bf16 MFMA, fp32 accumulation: the exact gradient
// of the bf16 engine's own patch embedding.  `copies` stacked copies of each image's rows are summed in the accumulators in the order
// s = 0, 1, ... (integrated gradients fold their interpolants here), then scaled once and either stored or added to what d_images holds.
//
// patch_embed_dgrad_kernel: grid (G, 3), one workgroup of 16 waves per (row range, channel c), one workgroup per CU (LDS).
//   The channel's 192 x 256 weight slab is staged into LDS TRANSPOSED (k-major, 400-byte rows), so that every MFMA A fragment -- 8
//   consecutive n of one pixel column k -- is one ds_read_b128.  Wave w owns the pixel rows ky = 4 (w & 3) .. +3 of the patch and the
//   patch rows r = r0 + (w >> 2), +4, ... of the workgroup's range.  Per patch row (b, py) the output tile is D[k][px] (16 k per MFMA
//   tile, px = 0..15 with 14 and 15 as zero padding): lane l holds kx = 4 (l >> 4) .. +3 of px = l & 15, so each ky row of the 14
//   patches is ONE float4 store per live lane -- 224 contiguous floats (896 bytes), a whole image row of the channel.
//   Nothing outside the B_out output images is written; dY rows beyond copies * B_out images are never read.
// Measured at batch 256 on MI355X (rocprofv3, tools/time_input_grad.py): 53 us for 19 MB of dY read and 154 MB of pixels written,
// 3.3 TB/s; the store stream bounds it.
#include <algorithm>

#include "common.h"

namespace {

constexpr int PE_T = 197, PE_D = 192, PE_PD = 768, PE_NP = 14, PE_IMG = 224;
constexpr int PE_WT_LD = PE_D + 8;                  // bf16 elements per LDS row of the transposed slab
constexpr int PE_WAVES = 16, PE_RG = PE_WAVES / 4;  // four pixel-row quarters x four patch-row groups
constexpr size_t PE_LDS = (size_t)256 * PE_WT_LD * 2;
constexpr int PE_MAX_WGS = 85;                      // x 3 channels: one workgroup per CU of the 256
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

struct PeDgradArgs {
  const bf16* dY; int ldy;
  const bf16* W;
  float* out;
  int b_out, copies, rows_per_wg, accumulate;
  float scale;
};

__global__ __launch_bounds__(PE_WAVES * 64) void patch_embed_dgrad_kernel(const PeDgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16 lds[];       // wt[k][n] = W[n][c 256 + k], k < 256, row stride PE_WT_LD
  const int c = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  // staging: item = (pair of rows n, n + 1; chunk of 8 columns) -> 8 dword stores of the two rows' values side by side
  unsigned int* lds32 = (unsigned int*)lds;
  for (int i = tid; i < (PE_D / 2) * 32; i += PE_WAVES * 64) {
    const int np = i % (PE_D / 2), kc = i / (PE_D / 2);
    const bf16* src = a.W + (size_t)(2 * np) * PE_PD + c * 256 + kc * 8;
    // (read as 16-bit integers: per-element __builtin_bit_cast of the loaded __bf16 vector staged element 0 for every j)
    const u16x8 v0 = *(const u16x8*)src;
    const u16x8 v1 = *(const u16x8*)(src + PE_PD);
#pragma unroll
    for (int j = 0; j < 8; ++j) lds32[((kc * 8 + j) * PE_WT_LD) / 2 + np] = (unsigned int)v0[j] | ((unsigned int)v1[j] << 16);
  }
  __syncthreads();
  const int kq = wave & 3, rg = wave >> 2;
  const bf16* wrow = lds + (size_t)(kq * 64 + l15) * PE_WT_LD + lg * 8;     // + t 16 rows + ks 32 columns
  const int R = a.b_out * PE_NP;
  const int r0 = blockIdx.x * a.rows_per_wg;
  const int r1 = min(R, r0 + a.rows_per_wg);
  const bool live = l15 < PE_NP;
  const int px = live ? l15 : 0;                       // padding lanes read a valid row and drop it (keep_if)
  for (int r = r0 + rg; r < r1; r += PE_RG) {
    const int b = r / PE_NP, py = r - b * PE_NP;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < a.copies; ++s) {
      // the W fragments are re-read from LDS for every copy: kept in registers they would take 96 VGPRs and spill at 4 waves per SIMD
      int woff = 0;
      asm volatile("" : "+v"(woff));
      const bf16* w = wrow + woff;
      const bf16* y = a.dY + ((size_t)(s * a.b_out + b) * PE_T + 1 + py * PE_NP + px) * a.ldy + lg * 8;
      bf16x8 yf[6];
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) yf[ks] = keep_if(*(const bf16x8*)(y + ks * 32), live);
#pragma unroll
      for (int ks = 0; ks < 6; ++ks)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = mfma16(*(const bf16x8*)(w + t * 16 * PE_WT_LD + ks * 32), yf[ks], acc[t]);   // D[k][px]
    }
    if (live) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ky = kq * 4 + t;
        float4* o = (float4*)(a.out + (((size_t)b * 3 + c) * PE_IMG + py * 16 + ky) * PE_IMG + px * 16 + lg * 4);
        float4 v = make_float4(acc[t][0] * a.scale, acc[t][1] * a.scale, acc[t][2] * a.scale, acc[t][3] * a.scale);
        if (a.accumulate) {
          const float4 p = *o;
          v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        *o = v;
      }
    }
  }
}

}  // namespace

extern "C" int rovit_patch_embed_dgrad(const void* dY, int ldy, const void* W, float* d_images, int b_out, int copies, float scale,
                                       int accumulate, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(dY && W && d_images, ROVIT_ERR_NULL, "patch_embed_dgrad: null pointer");
  ROVIT_CHECK_ARG(b_out > 0 && copies > 0 && (long)b_out * copies * PE_T <= (1L << 30), ROVIT_ERR_SHAPE,
                  "patch_embed_dgrad: bad batch %d / copies %d", b_out, copies);
  ROVIT_CHECK_ARG(ldy >= PE_D && ldy % 8 == 0 && rovit_aligned16(dY) && rovit_aligned16(W) && rovit_aligned16(d_images), ROVIT_ERR_ALIGN,
                  "patch_embed_dgrad: dY / W / d_images must be 16-byte aligned with ldy %% 8 == 0 and ldy >= 192");
  const int R = b_out * PE_NP;
  const int G = std::min((R + PE_RG - 1) / PE_RG, PE_MAX_WGS);
  PeDgradArgs a{(const bf16*)dY, ldy, (const bf16*)W, d_images, b_out, copies, (R + G - 1) / G, accumulate ? 1 : 0, scale};
  ROVIT_CHECK_ARG(rovit_set_max_lds((const void*)patch_embed_dgrad_kernel, PE_LDS), ROVIT_ERR_LAUNCH,
                  "patch_embed_dgrad: cannot raise the LDS limit");
  hipLaunchKernelGGL(patch_embed_dgrad_kernel, dim3(G, 3), dim3(PE_WAVES * 64), PE_LDS, (hipStream_t)stream, a);
  ROVIT_CHECK_LAUNCH("patch_embed_dgrad");
  return ROVIT_OK;
}
