// Last-layer Laplace approximation of the heads on the device: the pointwise GGN weights (rovit_laplace_weights), the weighted Gram
// matrices of the augmented hidden rows over every training row (rovit_laplace_gram), and the closed-form logit covariance and probit
// probabilities of query rows against the whitened posterior (rovit_laplace_predict).  Kristiadi et al., ICML 2020; Daxberger et al.,
// NeurIPS 2021.  The reference has no counterpart: its only epistemic figure is sampled (MC dropout).
//
// A head is fc1 (hid, E) + bias, ReLU, last layer.  a = [relu(fc1 f + b1); 1; 0 ...] is the augmented hidden row, padded from D = hid + 1
// to P = hid + 32 columns with exact zeros (a row that is left out is zero in every column, the 1 included: exact zero products).
// The Grams and the whitening run on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32) on the tiles of feature_tiles.h, which
// density.hip's two matrix kernels share; the small fc1 product in front of them is accumulated in fp64 (lap_hidden says why).
//
// rovit_laplace_gram, three kernels on the caller's stream; a chunk is R = lap_chunk_rows(n) consecutive rows (a function of n alone):
//   lap_rows_kernel   per 64-row tile: the feature rows into LDS, is any feature or weight of a row non-finite, the hidden rows
//                     (lap_hidden: fp64 accumulation, one rounding) and from there to the workspace (n, P) with the row flags and the tile's count of bad rows.
//   lap_gram_kernel   per (chunk, k): 32-row slabs of A into LDS, A^T (w_k A) of the upper tile triangle, the rows of the chunk in order
//                     along k of the matrix instruction; each wave keeps its tiles' accumulators over the whole chunk and writes them out.
//   lap_fold_kernel   per element of the upper triangle of every G_k: the chunk partials in fp64 in chunk order, written to [a][b] and
//                     [b][a]; workgroup 0 adds the tiles' integer counts and writes the header.
// rovit_laplace_predict, one kernel: a workgroup stages 64 feature rows, forms their hidden rows in LDS (lap_hidden), then streams W: per
//   class block t and pair of its 32-row tiles (one per wave pair), per class block c <= t the tile's columns of block c into LDS (up to
//   the diagonal tile for c = t) and z_c on the matrix instruction, one query row per lane; then S[c][d] += z_c z_d in-lane.
// Work items are walked with a stride of the grid, and no item's result depends on which workgroup computes it.  No floating-point atomics.
#include "common.h"
#include "feature_tiles.h"
#include "laplace_device.h"

namespace {

using namespace ftile;                  // tile_dot, upper_tiles, wave_tiles, gram_slab, store_acc_tile, fold_element
using namespace laplace;                // NT, MAXC, ROWS, lap_hidden, lap_stage_features: shared with influence.hip
constexpr int SLAB = 32;                // rows of one LDS slab of the gram pass
constexpr int MAXK = ROVIT_LAPLACE_MAX_WEIGHTS;
static_assert(MAXK == MAXC * (MAXC + 1) / 2, "one weight per pair of classes");

inline int lap_chunk_rows(int n) { return 256 * ((n + 256 * ROVIT_LAPLACE_MAX_CHUNKS - 1) / (256 * ROVIT_LAPLACE_MAX_CHUNKS)); }

// ---- weights -------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NT) void lap_weights_kernel(const rovit_laplace_weight_args a) {
  const int C = a.num_classes, K = C * (C + 1) / 2, lane = threadIdx.x & 63;
  const int rounds = (a.n + NT * (int)gridDim.x - 1) / (NT * (int)gridDim.x);
  for (int it = 0; it < rounds; ++it) {                        // every lane runs every round: the ballots see whole waves
    const int i = (it * (int)gridDim.x + (int)blockIdx.x) * NT + (int)threadIdx.x;
    bool bad_l = false, bad_v = false;
    if (i < a.n && a.cls_logits) {
      const float* lg = a.cls_logits + (size_t)i * C;
      double e[MAXC];
      double m = 0.0;
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < C) {
          const float l = lg[c];
          bad_l |= !isfinite(l);
          e[c] = (double)l;
          m = c == 0 ? e[c] : (e[c] > m ? e[c] : m);
        }
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < C) {
          e[c] = bad_l ? 0.0 : exp(e[c] - m);
          s += e[c];
        }
      const double inv = bad_l ? 0.0 : 1.0 / (s * s);
      float* out = a.cls_weights + (size_t)i * K;
      int k = 0;
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < C) {
          double rest = 0.0;
#pragma unroll
          for (int d = 0; d < MAXC; ++d)
            if (d < C && d != c) rest += e[d];
          out[k++] = bad_l ? 0.f : (float)(e[c] * rest * inv);
#pragma unroll
          for (int d = 0; d < MAXC; ++d)
            if (d > c && d < C) out[k++] = bad_l ? 0.f : (float)(-(e[c] * e[d]) * inv);
        }
    }
    if (i < a.n && a.log_var) {
      const float v = a.log_var[i];
      const float w = (float)exp(-(double)v);
      bad_v = !isfinite(v) || !isfinite(w);
      a.mu_weights[i] = bad_v ? 0.f : w;
    }
    const unsigned long long nl = __popcll(__ballot(bad_l)), nv = __popcll(__ballot(bad_v));
    if (lane == 0) {
      if (nl) atomicAdd((unsigned long long*)&a.counts[ROVIT_LAPLACE_BAD_LOGITS], nl);
      if (nv) atomicAdd((unsigned long long*)&a.counts[ROVIT_LAPLACE_BAD_LOG_VAR], nv);
    }
  }
}

// ---- gram ----------------------------------------------------------------------------------------------------------------------------

struct GramLayout { size_t rows, flag, bad, part, total; };
inline GramLayout gram_layout(int n, int hid, int K) {
  const size_t R = lap_chunk_rows(n), chunks = ((size_t)n + R - 1) / R, P = hid + 32, tiles = ((size_t)n + ROWS - 1) / ROWS;
  GramLayout l;
  l.rows = 0;
  l.flag = l.rows + rovit_up16((size_t)n * P * 4);
  l.bad = l.flag + rovit_up16((size_t)n * 4);
  l.part = l.bad + rovit_up16(tiles * 4);
  l.total = l.part + rovit_up16(chunks * K * upper_tiles((int)(P / 32)) * 1024 * 4);
  return l;
}

struct GramArgs {
  int n, E, hid, K, R, chunks;
  const float* x;
  const float* w1;
  const float* b1;
  const float* w;           // (n, K)
  float* rows;              // (n, P): the padded augmented hidden rows, zeros for a row that is left out
  int* flag;                // (n): 1 valid, 0 left out
  int* bad;                 // (tiles of 64 rows): rows left out
  float* part;              // (chunks, K, tiles, 32, 32)
  void* result;
};

inline size_t rows_lds_bytes(int E, int hid) { return ((size_t)ROWS * (E + 4) + (size_t)ROWS * (hid + 36) + ROWS) * 4; }

__global__ __launch_bounds__(NT) void lap_rows_kernel(const GramArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int E = a.E, hid = a.hid, K = a.K, n = a.n, P = hid + 32, SA = hid + 36, ST = E + 4, P4 = P / 4;
  float* Fs = lds;                                              // [64][ST]
  float* As = Fs + ROWS * ST;                                   // [64][SA]
  int* s_ok = (int*)(As + ROWS * SA);                           // [64]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tiles = (n + ROWS - 1) / ROWS;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = tile * ROWS;
    __syncthreads();
    lap_stage_features(Fs, a.x, r0, n, E);
    for (int rr = 0; rr < 16; ++rr) {                           // a wave per row: is any feature or weight non-finite?
      const int lr = wv * 16 + rr, row = r0 + lr;
      bool bad = false;
      if (row < n) {
        for (int e = lane; e < E; e += 64) bad |= !isfinite(a.x[(size_t)row * E + e]);
        for (int k = lane; k < K; k += 64) bad |= !isfinite(a.w[(size_t)row * K + k]);
      }
      const bool any_bad = __ballot(bad) != 0ull;
      if (lane == 0) s_ok[lr] = (row < n && !any_bad) ? 1 : 0;
    }
    __syncthreads();
    lap_hidden(Fs, As, s_ok, a.w1, a.b1, E, hid);
    if (tid < ROWS) {
      const bool in = r0 + tid < n;
      if (in) a.flag[r0 + tid] = s_ok[tid];
      const unsigned long long left_out = __ballot(in && s_ok[tid] == 0);
      if (tid == 0) a.bad[tile] = (int)__popcll(left_out);
    }
    __syncthreads();
    for (int idx = tid; idx < ROWS * P4; idx += NT) {
      const int row = idx / P4, c4 = idx - row * P4;
      if (r0 + row < n) *reinterpret_cast<float4*>(a.rows + (size_t)(r0 + row) * P + 4 * c4) = *reinterpret_cast<const float4*>(As + row * SA + 4 * c4);
    }
  }
}

struct Scaled {                 // gram_slab's B operand: w_k of the slab row times the row
  float wk;
  __device__ __forceinline__ float operator()(float x) const { return wk * x; }
};
struct WeightedRows {
  const float* w;              // [SLAB]
  __device__ __forceinline__ Scaled operator()(int row) const { return Scaled{w[row]}; }
};

template <int TP>
__global__ __launch_bounds__(NT) void lap_gram_kernel(const GramArgs a) {
  constexpr int P = 32 * TP, TILES = upper_tiles(TP), NQ = (TILES + 3) / 4;
  __shared__ __attribute__((aligned(16))) float Xs[SLAB * P];
  __shared__ float s_w[SLAB];
  const int tid = threadIdx.x, n = a.n, K = a.K;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  int ti[NQ], tj[NQ];
  wave_tiles<TP>(wv, ti, tj);
  const int items = a.chunks * K;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int chunk = w / K, k = w - chunk * K;
    f32x16 acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    for (int s0 = 0; s0 < a.R; s0 += SLAB) {
      const int rb = chunk * a.R + s0;
      if (rb >= n) break;
      __syncthreads();
#pragma unroll
      for (int it = 0; it < TP; ++it) {                         // SLAB * P / 4 = 256 TP float4
        const int idx = tid + NT * it, row = idx / (P / 4), c4 = idx - row * (P / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rb + row < n) v = *reinterpret_cast<const float4*>(a.rows + (size_t)(rb + row) * P + 4 * c4);
        *reinterpret_cast<float4*>(Xs + row * P + 4 * c4) = v;
      }
      if (tid < SLAB) {
        const int gr = rb + tid;
        s_w[tid] = (gr < n && a.flag[gr] != 0) ? a.w[(size_t)gr * K + k] : 0.f;   // a row that is left out: 0, whatever its weight
      }
      __syncthreads();
      gram_slab<TP>(acc, Xs, wv, ti, tj, WeightedRows{s_w});     // k = the rows of the chunk in order
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (wv + 4 * q < TILES) store_acc_tile(a.part + ((size_t)w * TILES + (wv + 4 * q)) * 1024, acc[q]);
  }
}

__global__ __launch_bounds__(NT) void lap_fold_kernel(const GramArgs a) {
  __shared__ unsigned long long s_u[4];
  const int D = a.hid + 1, TP = (a.hid + 32) / 32, tiles = upper_tiles(TP), K = a.K, items = K * tiles * 4;
  if (blockIdx.x == 0) {
    unsigned long long bad = 0;
    const int row_tiles = (a.n + ROWS - 1) / ROWS;
    for (int t = threadIdx.x; t < row_tiles; t += NT) bad += (unsigned long long)a.bad[t];
    bad = block_sum_t(bad, s_u);
    if (threadIdx.x == 0) {
      long long* head = (long long*)a.result;
      for (int i = 0; i < ROVIT_LAPLACE_HEADER; ++i) head[i] = 0;
      head[ROVIT_LAPLACE_N] = a.n;
      head[ROVIT_LAPLACE_N_VALID] = a.n - (long long)bad;
      head[ROVIT_LAPLACE_BAD_ROWS] = (long long)bad;
    }
  }
  double* G = (double*)a.result + ROVIT_LAPLACE_HEADER;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int k = w / (tiles * 4), rem = w - k * tiles * 4;
    const int q = rem >> 2, el = (rem & 3) * NT + threadIdx.x;
    int ra, rb;
    if (fold_element(q, el, TP, ra, rb) || ra >= D || rb >= D) continue;   // the mirror fills the lower half; the padding is not part of G
    double s = 0.0;
    for (int c = 0; c < a.chunks; ++c) s += (double)a.part[(((size_t)c * K + k) * tiles + q) * 1024 + el];
    double* Gk = G + (size_t)k * D * D;
    Gk[(size_t)ra * D + rb] = s;
    Gk[(size_t)rb * D + ra] = s;
  }
}

// ---- predict -------------------------------------------------------------------------------------------------------------------------

// As [64][SA], then a region that holds the feature rows first and the two W tiles afterwards, then the row flags
inline size_t predict_lds_bytes(int E, int hid) {
  return ((size_t)ROWS * (hid + 36) + lap_stream_region(E, hid) + ROWS) * 4;
}

__global__ __launch_bounds__(NT) void lap_predict_kernel(const rovit_laplace_query a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int E = a.embed, hid = a.hid, C = a.num_classes, B = a.batch, P = hid + 32, SA = hid + 36, TP = P / 32, P4 = P / 4;
  const int N = C * P;                                          // W is (N, N)
  const int region = (int)lap_stream_region(E, hid);
  float* As = lds;                                              // [64][SA] augmented hidden rows
  float* Fs = As + ROWS * SA;                                   // [64][E + 4] feature rows, then
  float* Ws = Fs;                                               // [2][32][SA] one tile of W per wave pair, then the exchange of S
  int* s_ok = (int*)(Fs + region);                              // [64]
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), rt = wv & 1, th = wv >> 1;
  const int tiles = (B + ROWS - 1) / ROWS;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = tile * ROWS;
    __syncthreads();
    lap_stage_features(Fs, a.features, r0, B, E);
    if (tid < ROWS) s_ok[tid] = r0 + tid < B ? 1 : 0;
    __syncthreads();
    lap_hidden(Fs, As, s_ok, a.fc1_weight, a.fc1_bias, E, hid);
    float S[MAXK];
#pragma unroll
    for (int q = 0; q < MAXK; ++q) S[q] = 0.f;
    const float* frow = As + (rt * 32 + l31) * SA + 4 * lh;     // B[k][n = row]
    const float* wrow = Ws + (th * 32 + l31) * SA + 4 * lh;     // A[m = t][k]: plain rows, lane half h holds k = kk + 4 h + s in step s
    for (int cb = 0; cb < C; ++cb) {
      for (int at0 = 0; at0 < TP; at0 += 2) {
        const int at = at0 + th;                                // this wave's tile of class block cb
        const bool live = at < TP;
        f32x16 acc[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c <= cb) {                                        // uniform over the workgroup
            __syncthreads();                                    // the first one also closes lap_hidden's writes and Fs' reads
            for (int idx = tid; idx < 64 * P4; idx += NT) {     // rows of tiles at0, at0 + 1 of block cb, columns of block c
              const int row = idx / P4, c4 = idx - row * P4, t2 = at0 + (row >> 5);
              const int kend2 = c == cb ? 32 * t2 + 32 : P;
              if (t2 < TP && 4 * c4 < kend2)
                *reinterpret_cast<float4*>(Ws + row * SA + 4 * c4) =
                    *reinterpret_cast<const float4*>(a.whitening + (size_t)(cb * P + 32 * t2 + (row & 31)) * N + (size_t)c * P + 4 * c4);
            }
            __syncthreads();
            if (live) {
              const int kend = c == cb ? 32 * at + 32 : P;
              acc[c] = tile_dot(acc[c], wrow, frow, kend);
            }
          }
        // lane (l31, h) holds z_c[row l31][t = 32 at + acc_row(r, h)] of every c <= cb
        if (live) {
          int q = 0;
#pragma unroll
          for (int c = 0; c < MAXC; ++c)
#pragma unroll
            for (int d = c; d < MAXC; ++d, ++q)
              if (d <= cb) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) s = fmaf(acc[c][r], acc[d][r], s);
                S[q] += s;
              }
        }
      }
    }
    // S[q], q over the MAXC triangle: add the lane halves, then the two wave pairs (th = 0 first)
#pragma unroll
    for (int q = 0; q < MAXK; ++q) S[q] += __shfl_xor(S[q], 32);
    __syncthreads();                                            // Ws is free
    float* Sx = Ws;                                             // [MAXK][64]
    if (th == 1 && lh == 0) {
#pragma unroll
      for (int q = 0; q < MAXK; ++q) Sx[q * ROWS + rt * 32 + l31] = S[q];
    }
    __syncthreads();
    const int row = r0 + rt * 32 + l31;
    if (th == 0 && lh == 0 && row < B) {
      float var[MAXC];
      int q = 0;
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
#pragma unroll
        for (int d = c; d < MAXC; ++d, ++q)
          if (d < C) {
            const float s = S[q] + Sx[q * ROWS + rt * 32 + l31];
            a.logit_cov[((size_t)row * C + c) * C + d] = s;
            a.logit_cov[((size_t)row * C + d) * C + c] = s;
            if (c == d) {
              var[c] = s;
              a.logit_var[(size_t)row * C + c] = s;
            }
          }
      if (a.cls_logits) {
        // fp64: t_c = l_c / sqrt(1 + (pi / 8) S_cc), probs = softmax(t), confidence_score = rest / sum over all but the first maximum
        const float* lg = a.cls_logits + (size_t)row * C;
        double t[MAXC];
        double m = 0.0, mean = 0.0;
        int am = 0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) {
            t[c] = (double)lg[c] / sqrt(1.0 + 0.39269908169872415481 * (double)var[c]);
            mean += (double)var[c];
            if (c == 0 || t[c] > m) { m = t[c]; am = c; }
          }
        double sum = 0.0, rest = 0.0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) {
            t[c] = exp(t[c] - m);
            sum += t[c];
            if (c != am) rest += t[c];
          }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) a.probs[(size_t)row * C + c] = (float)(t[c] / sum);
        a.confidence_score[row] = (float)(rest / sum);
        a.mean_logit_var[row] = (float)(mean / (double)C);
      }
    }
  }
}

inline bool gram_limits_ok(int n, int E, int hid, int K) {
  return n >= 1 && n <= ROVIT_KAN_STATS_MAX_ROWS && E >= 32 && E <= 256 && E % 32 == 0 && hid >= 32 && hid <= 256 && hid % 32 == 0 && K >= 1 &&
         K <= MAXK;
}

template <int TP>
void launch_gram(dim3 grid, hipStream_t s, const GramArgs& a) {
  hipLaunchKernelGGL(lap_gram_kernel<TP>, grid, dim3(NT), 0, s, a);
}

}  // namespace

extern "C" int rovit_laplace_weights(const rovit_laplace_weight_args* p, rovit_stream_t stream) {
  const char* who = "laplace_weights";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_KAN_STATS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_KAN_STATS_MAX_ROWS);
  ROVIT_CHECK_ARG(p->num_classes >= 1 && p->num_classes <= MAXC, ROVIT_ERR_SHAPE, "%s: %d classes (1..%d)", who, p->num_classes, MAXC);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->cls_logits || p->log_var, ROVIT_ERR_NULL, "%s: neither logits nor log_var", who);
  ROVIT_CHECK_ARG((!p->cls_logits || p->cls_weights) && (!p->log_var || p->mu_weights) && p->counts, ROVIT_ERR_NULL,
                  "%s: an output is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->cls_logits, 4) && rovit_aligned(p->log_var, 4) && rovit_aligned(p->cls_weights, 4) &&
                      rovit_aligned(p->mu_weights, 4) && rovit_aligned(p->counts, 8),
                  ROVIT_ERR_ALIGN, "%s: an array is not aligned to its element size", who);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(p->counts, 0, ROVIT_LAPLACE_COUNT_WORDS * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(lap_weights_kernel, rovit_grid(((long long)p->n + NT - 1) / NT, p->max_workgroups), dim3(NT), 0, s, *p);
  ROVIT_CHECK_LAUNCH("lap_weights_kernel");
  return ROVIT_OK;
}

extern "C" size_t rovit_laplace_workspace_bytes(int n, int E, int hid, int K) {
  return gram_limits_ok(n, E, hid, K) ? gram_layout(n, hid, K).total : 0;
}

extern "C" int rovit_laplace_gram(const rovit_laplace_fit* p, rovit_stream_t stream) {
  const char* who = "laplace_gram";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_KAN_STATS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_KAN_STATS_MAX_ROWS);
  ROVIT_CHECK_ARG(p->embed >= 32 && p->embed <= 256 && p->embed % 32 == 0, ROVIT_ERR_SHAPE, "%s: embed %d (a multiple of 32 in 32..256)", who,
                  p->embed);
  ROVIT_CHECK_ARG(p->hid >= 32 && p->hid <= 256 && p->hid % 32 == 0, ROVIT_ERR_SHAPE, "%s: hid %d (a multiple of 32 in 32..256)", who, p->hid);
  ROVIT_CHECK_ARG(p->num_weights >= 1 && p->num_weights <= MAXK, ROVIT_ERR_SHAPE, "%s: %d weight columns (1..%d)", who, p->num_weights, MAXK);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->features && p->fc1_weight && p->fc1_bias && p->weights && p->workspace && p->result, ROVIT_ERR_NULL, "%s: a null pointer", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->features) && rovit_aligned16(p->fc1_weight) && rovit_aligned(p->fc1_bias, 4) && rovit_aligned(p->weights, 4) &&
                      rovit_aligned16(p->workspace) && rovit_aligned(p->result, 8),
                  ROVIT_ERR_ALIGN, "%s: the features, fc1_weight or the workspace are not 16-byte aligned, or another array not to its words", who);
  const int n = p->n, E = p->embed, hid = p->hid, K = p->num_weights;
  const GramLayout l = gram_layout(n, hid, K);
  ROVIT_CHECK_ARG(p->workspace_bytes >= l.total, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes,
                  l.total);
  const size_t lds = rows_lds_bytes(E, hid);
  ROVIT_CHECK_ARG(rovit_set_max_lds((const void*)lap_rows_kernel, lds), ROVIT_ERR_LAUNCH, "%s: cannot raise the LDS limit", who);
  char* ws = (char*)p->workspace;
  GramArgs a;
  a.n = n; a.E = E; a.hid = hid; a.K = K; a.R = lap_chunk_rows(n); a.chunks = (n + a.R - 1) / a.R;
  a.x = p->features; a.w1 = p->fc1_weight; a.b1 = p->fc1_bias; a.w = p->weights;
  a.rows = (float*)(ws + l.rows);
  a.flag = (int*)(ws + l.flag);
  a.bad = (int*)(ws + l.bad);
  a.part = (float*)(ws + l.part);
  a.result = p->result;
  hipStream_t s = (hipStream_t)stream;
  auto grid = [&](long long items) { return rovit_grid(items, p->max_workgroups); };
  const int TP = (hid + 32) / 32;
  hipLaunchKernelGGL(lap_rows_kernel, grid(((long long)n + ROWS - 1) / ROWS), dim3(NT), lds, s, a);
  ROVIT_CHECK_LAUNCH("lap_rows_kernel");
  const dim3 g = grid((long long)a.chunks * K);
  switch (TP) {
    case 2: launch_gram<2>(g, s, a); break;
    case 3: launch_gram<3>(g, s, a); break;
    case 4: launch_gram<4>(g, s, a); break;
    case 5: launch_gram<5>(g, s, a); break;
    case 6: launch_gram<6>(g, s, a); break;
    case 7: launch_gram<7>(g, s, a); break;
    case 8: launch_gram<8>(g, s, a); break;
    default: launch_gram<9>(g, s, a); break;
  }
  ROVIT_CHECK_LAUNCH("lap_gram_kernel");
  hipLaunchKernelGGL(lap_fold_kernel, grid(4ll * K * upper_tiles(TP)), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("lap_fold_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_laplace_predict(const rovit_laplace_query* p, rovit_stream_t stream) {
  const char* who = "laplace_predict";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->batch >= 1, ROVIT_ERR_SHAPE, "%s: batch %d (>= 1)", who, p->batch);
  ROVIT_CHECK_ARG(p->embed >= 32 && p->embed <= 256 && p->embed % 32 == 0, ROVIT_ERR_SHAPE, "%s: embed %d (a multiple of 32 in 32..256)", who,
                  p->embed);
  ROVIT_CHECK_ARG(p->hid >= 32 && p->hid <= 256 && p->hid % 32 == 0, ROVIT_ERR_SHAPE, "%s: hid %d (a multiple of 32 in 32..256)", who, p->hid);
  ROVIT_CHECK_ARG(p->num_classes >= 1 && p->num_classes <= MAXC, ROVIT_ERR_SHAPE, "%s: %d classes (1..%d)", who, p->num_classes, MAXC);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->features && p->fc1_weight && p->fc1_bias && p->whitening, ROVIT_ERR_NULL,
                  "%s: the features, fc1 or the whitening table are missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->logit_cov && p->logit_var, ROVIT_ERR_NULL, "%s: an output is missing (null pointer)", who);
  ROVIT_CHECK_ARG(!p->cls_logits || (p->probs && p->confidence_score && p->mean_logit_var), ROVIT_ERR_NULL,
                  "%s: logits without the probs, confidence_score and mean_logit_var outputs", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->features) && rovit_aligned16(p->fc1_weight) && rovit_aligned16(p->whitening), ROVIT_ERR_ALIGN,
                  "%s: the features, fc1_weight or the whitening matrix are not 16-byte aligned", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->fc1_bias, 4) && rovit_aligned(p->cls_logits, 4) && rovit_aligned(p->logit_cov, 4) &&
                      rovit_aligned(p->logit_var, 4) && rovit_aligned(p->probs, 4) && rovit_aligned(p->confidence_score, 4) &&
                      rovit_aligned(p->mean_logit_var, 4),
                  ROVIT_ERR_ALIGN, "%s: an array is not aligned to its element size", who);
  const size_t lds = predict_lds_bytes(p->embed, p->hid);
  ROVIT_CHECK_ARG(rovit_set_max_lds((const void*)lap_predict_kernel, lds), ROVIT_ERR_LAUNCH, "%s: cannot raise the LDS limit", who);
  const long long tiles = ((long long)p->batch + ROWS - 1) / ROWS;
  hipLaunchKernelGGL(lap_predict_kernel, rovit_grid(tiles, p->max_workgroups), dim3(NT), lds, (hipStream_t)stream, *p);
  ROVIT_CHECK_LAUNCH("lap_predict_kernel");
  return ROVIT_OK;
}
