// PatchDropout (Liu et al., WACV 2023) for the training step: the per-sample draw of the kept patches and the scatter that takes the
// short sequences' gradient rows back to the 197-token layout (rovit_vit_forward_train_tokens / rovit_vit_backward_tokens, vit.hip).
//
// Draw.  One workgroup per sample, thread p < 196 owns patch p.  Its key is one word of Philox4x32-10 (philox.h lists the counter); the
// 196 keys go to LDS and every thread counts the pairs (key, patch) below its own (rank_count.h).  The ranks are a permutation of
// 0..195 whatever the keys are, so rank < k keeps exactly k patches, and a uniformly random permutation's first k are a uniformly random
// subset.  A kept patch's place in the ascending list is the number of kept patches below it, counted from the LDS flags in index
// order.  Integer compares and fixed loops only: the output is a pure function of (seed, step, b, k).
//
// Scatter.  One thread per 16 bytes of the dense buffer (24 per 384-byte bf16 row): it looks its token up in inv and stores either the
// short sequence's 16 bytes or zeros, so every dense byte is written exactly once and nothing has to be cleared first.
#include "common.h"
#include "philox.h"
#include "rank_count.h"

namespace {

constexpr int PT = 197, PP = 196, PV = 192 * 2 / 16;     // tokens, patches, 16-byte vectors per bf16 row

__global__ __launch_bounds__(256) void patch_dropout_draw_kernel(unsigned long long seed, unsigned step_lo, unsigned step_hi, int* __restrict__ keep,
                                                                 int* __restrict__ src, int* __restrict__ inv, int k) {
  __shared__ unsigned sW[PP];
  __shared__ unsigned sKept[PP];
  const int b = blockIdx.x, p = threadIdx.x;
  unsigned w = 0;
  if (p < PP) {
    const U4 r = philox4x32_10(seed, (unsigned)b, ROVIT_PATCH_DROPOUT_STREAM + (unsigned)(p >> 2), step_lo, step_hi);
    const int q = p & 3;
    w = q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w;
    sW[p] = w;
  }
  __syncthreads();
  unsigned kept = 0;
  if (p < PP) {
    kept = rank_count_pairs_u32(sW, PP, w, p) < (unsigned)k;
    sKept[p] = kept;
  }
  __syncthreads();
  if (p == 0) {                     // the class token: row 0 of every short sequence
    src[(size_t)b * (k + 1)] = 0;
    inv[(size_t)b * PT] = 0;
  }
  if (p < PP) {
    int pos = 0;
    for (int j = 0; j < p; ++j) pos += (int)sKept[j];
    // pos < k for a kept patch: the k kept flags below and at p number at most k (the ranks are a permutation)
    if (kept && pos < k) {
      keep[(size_t)b * k + pos] = p;
      src[(size_t)b * (k + 1) + 1 + pos] = 1 + p;
    }
    inv[(size_t)b * PT + 1 + p] = kept ? 1 + pos : -1;
  }
}

struct ScatterArgs {
  const uint4* rows;
  const int* inv;
  uint4* dense;
  int tokens;
  unsigned total;                  // batch * 197 * PV  (< 2^31, checked on the host)
};

__global__ __launch_bounds__(256) void scatter_token_rows_kernel(const ScatterArgs a) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.total) return;
  const unsigned row = i / PV, c = i - row * PV;        // row = b * 197 + t
  const unsigned b = row / PT;
  const int r = a.inv[row];
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  // an index outside the short sequence reads nothing: the row is zeros, as a dropped token's
  if (r >= 0 && r < a.tokens) v = a.rows[((size_t)b * a.tokens + r) * PV + c];
  a.dense[i] = v;
}

}  // namespace

extern "C" int rovit_patch_dropout_draw(unsigned long long seed, unsigned long long step, int* keep, int* src, int* inv, int batch, int k,
                                        rovit_stream_t stream) {
  ROVIT_CHECK_ARG(keep && src && inv, ROVIT_ERR_NULL, "patch_dropout_draw: null keep / src / inv");
  ROVIT_CHECK_ARG(batch > 0 && batch <= (1 << 20), ROVIT_ERR_SHAPE, "patch_dropout_draw: batch must be in [1, 2^20], got %d", batch);
  ROVIT_CHECK_ARG(k >= 1 && k <= PP, ROVIT_ERR_SHAPE, "patch_dropout_draw: k must be in [1, %d], got %d", PP, k);
  hipLaunchKernelGGL(patch_dropout_draw_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, seed, (unsigned)step, (unsigned)(step >> 32), keep,
                     src, inv, k);
  ROVIT_CHECK_LAUNCH("patch_dropout_draw");
  return ROVIT_OK;
}

extern "C" int rovit_scatter_token_rows(const void* rows, const int* inv, void* dense, int batch, int tokens, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(rows && inv && dense, ROVIT_ERR_NULL, "scatter_token_rows: null rows / inv / dense");
  ROVIT_CHECK_ARG(batch > 0 && tokens >= 1 && tokens <= PT && (long)batch * PT * PV < (1L << 31), ROVIT_ERR_SHAPE,
                  "scatter_token_rows: bad batch %d / tokens %d", batch, tokens);
  ROVIT_CHECK_ARG(rovit_aligned16(rows) && rovit_aligned16(dense), ROVIT_ERR_ALIGN, "scatter_token_rows: rows and dense must be 16-byte aligned");
  ScatterArgs a{(const uint4*)rows, inv, (uint4*)dense, tokens, (unsigned)((long)batch * PT * PV)};
  hipLaunchKernelGGL(scatter_token_rows_kernel, dim3((a.total + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  ROVIT_CHECK_LAUNCH("scatter_token_rows");
  return ROVIT_OK;
}
