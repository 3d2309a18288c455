// Token-row gather of the deletion / insertion curves (rovit_vit_forward_tokens and, for sequences of different lengths in one call,
// rovit_vit_forward_ragged; vit.hip).
//
// The patch embedding is a 16x16 convolution with stride 16, so each token row depends on its own patch alone: every row of an image
// perturbed patch by patch is a row of the clean image's token table or of its baseline's (rovit_vit_embed writes both once).  This
// kernel builds the residual stream X of n_seq perturbed sequences of `tokens` rows from those tables:
//
//   X[s, r, :] = v >= 0 ? img[seq_img[s], v, :] : base[base_shared ? 0 : seq_img[s], -1 - v, :],   v = src[s * tokens + r]
//
// One thread per 16-byte quarter-column group (48 per 768-byte row): one global_load_dwordx4 and one global_store_dwordx4, consecutive
// lanes on consecutive addresses of a row.  Pure bandwidth: 2 x 38.7 MB per 256 sequences of 197 rows.  Every index is clamped into
// its table (image into [0, n_img), row into [0, 197)), as attention.hip's stage_tile clamps its loads, so a malformed descriptor
// reads a wrong row of the tables but never outside them.
#include "common.h"

namespace {

constexpr int GT = 197, GV = 192 / 4;       // rows per table entry, float4 per row

struct GatherArgs {
  const float4* img;
  const float4* base;
  const int* seq_img;
  const int* src;
  float4* X;
  int n_img, base_shared, tokens;
  unsigned total;                          // n_seq * tokens * GV  (< 2^31, checked on the host)
};

__global__ __launch_bounds__(256) void gather_token_rows_kernel(const GatherArgs a) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.total) return;
  const unsigned row = i / GV, c = i - row * GV;
  const unsigned s = row / (unsigned)a.tokens;
  const int img = min(max(a.seq_img[s], 0), a.n_img - 1);
  const int v = a.src[row];
  const float4* t = v >= 0 ? a.img + ((size_t)img * GT + min(v, GT - 1)) * GV
                           : a.base + ((size_t)(a.base_shared ? 0 : img) * GT + min(-1 - v, GT - 1)) * GV;   // -1 - v >= 0 for v < 0
  a.X[i] = t[c];
}

// The same gather for a ragged batch (rovit_vit_forward_ragged): sequences of different lengths packed back to back, src one entry per
// packed row, off (n_seq + 1) the device copy of the sequence offsets.  A row finds its sequence by bisection (the last s with
// off[s] <= row; at most 18 probes of an array that sits in L2; it ends on some s in [0, n_seq) whatever the array holds), then the
// image and the table row are clamped as above.
struct RaggedGatherArgs {
  const float4* img;
  const float4* base;
  const int* seq_img;
  const int* src;
  const int* off;
  float4* X;
  int n_img, base_shared, n_seq;
  unsigned total;                          // total_rows * GV  (< 2^31, checked on the host)
};

__global__ __launch_bounds__(256) void gather_token_rows_ragged_kernel(const RaggedGatherArgs a) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.total) return;
  const unsigned row = i / GV, c = i - row * GV;
  int lo = 0, hi = a.n_seq - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.off[mid] <= (int)row) lo = mid; else hi = mid - 1;
  }
  const int img = min(max(a.seq_img[lo], 0), a.n_img - 1);
  const int v = a.src[row];
  const float4* t = v >= 0 ? a.img + ((size_t)img * GT + min(v, GT - 1)) * GV
                           : a.base + ((size_t)(a.base_shared ? 0 : img) * GT + min(-1 - v, GT - 1)) * GV;
  a.X[i] = t[c];
}

}  // namespace

int rovit_gather_token_rows_ragged(const float* img_tokens, const float* base_tokens, int n_img, int base_shared, const int* seq_img,
                                   const int* src, const int* off_dev, float* X, int n_seq, int total_rows, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(img_tokens && base_tokens && seq_img && src && off_dev && X, ROVIT_ERR_NULL, "gather_token_rows_ragged: null pointer");
  ROVIT_CHECK_ARG(n_img > 0 && n_seq > 0 && total_rows >= n_seq && (long)total_rows * GV < (1L << 31), ROVIT_ERR_SHAPE,
                  "gather_token_rows_ragged: bad n_img %d / n_seq %d / total_rows %d", n_img, n_seq, total_rows);
  ROVIT_CHECK_ARG(rovit_aligned16(img_tokens) && rovit_aligned16(base_tokens) && rovit_aligned16(X), ROVIT_ERR_ALIGN,
                  "gather_token_rows_ragged: token tables and X must be 16-byte aligned");
  RaggedGatherArgs a{(const float4*)img_tokens, (const float4*)base_tokens, seq_img, src, off_dev, (float4*)X, n_img, base_shared ? 1 : 0,
                     n_seq, (unsigned)((long)total_rows * GV)};
  hipLaunchKernelGGL(gather_token_rows_ragged_kernel, dim3((a.total + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  ROVIT_CHECK_LAUNCH("gather_token_rows_ragged");
  return ROVIT_OK;
}

int rovit_gather_token_rows(const float* img_tokens, const float* base_tokens, int n_img, int base_shared, const int* seq_img, const int* src,
                            float* X, int n_seq, int tokens, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(img_tokens && base_tokens && seq_img && src && X, ROVIT_ERR_NULL, "gather_token_rows: null pointer");
  ROVIT_CHECK_ARG(n_img > 0 && n_seq > 0 && tokens >= 1 && tokens <= GT && (long)n_seq * tokens * GV < (1L << 31), ROVIT_ERR_SHAPE,
                  "gather_token_rows: bad n_img %d / n_seq %d / tokens %d", n_img, n_seq, tokens);
  ROVIT_CHECK_ARG(rovit_aligned16(img_tokens) && rovit_aligned16(base_tokens) && rovit_aligned16(X), ROVIT_ERR_ALIGN,
                  "gather_token_rows: token tables and X must be 16-byte aligned");
  GatherArgs a{(const float4*)img_tokens, (const float4*)base_tokens, seq_img, src, (float4*)X, n_img, base_shared ? 1 : 0, tokens,
               (unsigned)((long)n_seq * tokens * GV)};
  hipLaunchKernelGGL(gather_token_rows_kernel, dim3((a.total + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  ROVIT_CHECK_LAUNCH("gather_token_rows");
  return ROVIT_OK;
}
