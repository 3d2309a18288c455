// Feature-space density on the device: class-conditional Gaussian moments of the backbone features (rovit_density_moments), the
// Mahalanobis / relative-Mahalanobis scores of feature rows against the fitted tables (rovit_density_score), and AUROC / AUPR / FPR@TPR of
// two score populations (rovit_ood_metrics).  Lee et al., NeurIPS 2018; Ren et al., 2021.  The reference has no counterpart: its heads
// read outputs['features'] and nothing asks how far a feature row lies from the training features.
//
// Everything matrix-shaped runs on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32: a k-ordered fp32 fma chain; the tiles
// are those of feature_tiles.h, which laplace.hip shares): the whitening of a near-singular covariance amplifies operand error by
// sqrt(cond), so bf16 operands are out.
//
// rovit_density_moments, four kernels on the caller's stream; a chunk is R = density_chunk_rows(n) consecutive rows (a function of n alone):
//   dens_sums_kernel     per chunk: each row's class (-1 bad label, -2 non-finite feature) into the workspace, the per-class column sums
//                        in fp64 in row order (thread = column, the class slots in LDS), the chunk's integer counts.
//   dens_means_kernel    one workgroup: the chunk sums and counts folded in chunk order; the class means, the global mean (classes in
//                        index order), the header; the class means rounded to fp32 for the second pass.
//   dens_scatter_kernel  per chunk: 32-row slabs centred on the fp32 class mean into LDS (rows left out become zeros: exact zero products),
//                        X^T X of the upper tile triangle on the fp32 MFMA, rows of the chunk in order along k; each wave keeps its tiles'
//                        accumulators over the whole chunk and writes them to the workspace.
//   dens_fold_kernel     per element of the upper triangle: the chunk partials in fp64 in chunk order, written to [a][b] and [b][a].
// rovit_density_score, one kernel: a workgroup stages 64 feature rows in LDS; per 32-row tile of W and W0 it stages the tile's columns up
//   to the diagonal (the zero upper triangle is never multiplied: exact zeros either way), waves 0-1 form z = W f of row tiles 0-1, waves
//   2-3 z0 = W0 f; the accumulators hold one feature row per lane, so ||z - M_c||^2 is an in-lane sum plus one cross-half add.
// rovit_ood_metrics, three kernels: counted ranks on the tile of rank_count.h (uint32, integer atomics over the split j range), the per-row
//   terms with fixed-tree chunk sums, one fold.  rovit_ood_metrics_ex with ROVIT_RANK_SORT replaces ood_rank_kernel only: both populations
//   are sorted (sort_rank.hip) and the four counts of every row come from binary searches in the two sorted key arrays.
// Work items are walked with a stride of the grid, and no item's result depends on which workgroup computes it.  No floating-point atomics.
#include "common.h"
#include "feature_tiles.h"
#include "rank_count.h"
#include "sort_device.h"

namespace {

using namespace ftile;                  // tile_dot, acc_row, upper_tiles, wave_tiles, gram_slab, store_acc_tile, fold_element

constexpr int NT = 256;                 // threads per workgroup
constexpr int SLAB = 32;                // rows of one centred LDS slab of the scatter pass
constexpr int MAXC = ROVIT_EVAL_MAX_CLASSES;
constexpr int MAX_CHUNKS = 256;         // the chunk length grows with n so that never more partials than this exist
constexpr int SCORE_ROWS = ROVIT_DENSITY_SCORE_TILE;
static_assert(SCORE_ROWS == 64, "two row tiles of 32 per workgroup");
static_assert(NT == RANK_NT, "rank_stage_tile strides by RANK_NT");

inline int density_chunk_rows(int n) { return ROVIT_DENSITY_CHUNK_ROWS * ((n + ROVIT_DENSITY_CHUNK_ROWS * MAX_CHUNKS - 1) / (ROVIT_DENSITY_CHUNK_ROWS * MAX_CHUNKS)); }

// ---- moments -------------------------------------------------------------------------------------------------------------------------

struct MomLayout { size_t cls, csum, ccnt, mean32, part, total; };
inline MomLayout mom_layout(int n, int E, int C) {
  const size_t R = density_chunk_rows(n), chunks = ((size_t)n + R - 1) / R;
  MomLayout l;
  l.cls = 0;
  l.csum = l.cls + rovit_up16((size_t)n * 4);
  l.ccnt = l.csum + rovit_up16(chunks * C * E * 8);
  l.mean32 = l.ccnt + rovit_up16(chunks * (C + 2) * 8);
  l.part = l.mean32 + rovit_up16((size_t)C * E * 4);
  l.total = l.part + rovit_up16(chunks * upper_tiles(E / 32) * 1024 * 4);
  return l;
}

struct MomArgs {
  int n, E, C, R, chunks;
  const float* x;
  const int* labels;
  int* cls;                 // (n): class, -1 label outside [0, C), -2 non-finite feature
  double* csum;             // (chunks, C, E)
  long long* ccnt;          // (chunks, C + 2): class counts, bad labels, bad rows
  float* mean32;            // (C, E)
  float* part;              // (chunks, tiles, 32, 32)
  void* result;
};

__global__ __launch_bounds__(NT) void dens_sums_kernel(const MomArgs a) {
  __shared__ double s_sum[MAXC * 256];
  __shared__ int s_cls[NT];
  __shared__ unsigned s_cnt[MAXC + 2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = a.n, E = a.E, C = a.C;
  for (int w = blockIdx.x; w < a.chunks; w += gridDim.x) {
    __syncthreads();
    for (int k = tid; k < C * E; k += NT) s_sum[k] = 0.0;
    if (tid < MAXC + 2) s_cnt[tid] = 0;
    for (int sub = 0; sub < a.R; sub += NT) {
      const int r0 = w * a.R + sub;
      if (r0 >= n) break;
      __syncthreads();
      for (int rr = 0; rr < 64; ++rr) {                       // a wave per row: is any feature non-finite?
        const int row = r0 + wv * 64 + rr;
        if (row >= n) {
          if (lane == 0) s_cls[wv * 64 + rr] = -1;
          continue;
        }
        bool bad = false;
        for (int e = lane; e < E; e += 64) bad |= !isfinite(a.x[(size_t)row * E + e]);
        const bool any_bad = __ballot(bad) != 0ull;
        if (lane == 0) {
          const int lab = a.labels[row];
          const int c = (lab < 0 || lab >= C) ? -1 : (any_bad ? -2 : lab);
          s_cls[wv * 64 + rr] = c;
          a.cls[row] = c;
          atomicAdd(&s_cnt[c >= 0 ? c : (c == -1 ? C : C + 1)], 1u);
        }
      }
      __syncthreads();
      if (tid < E) {
        const int rows = min(NT, n - r0);
        for (int r = 0; r < rows; ++r) {
          const int c = s_cls[r];
          if (c >= 0) s_sum[c * E + tid] += (double)a.x[(size_t)(r0 + r) * E + tid];
        }
      }
    }
    __syncthreads();
    for (int k = tid; k < C * E; k += NT) a.csum[(size_t)w * C * E + k] = s_sum[k];
    if (tid < C + 2) a.ccnt[(size_t)w * (C + 2) + tid] = (long long)s_cnt[tid];
  }
}

__global__ __launch_bounds__(NT) void dens_means_kernel(const MomArgs a) {
  __shared__ long long s_tot[MAXC + 2];
  const int tid = threadIdx.x, E = a.E, C = a.C;
  long long* head = (long long*)a.result;
  double* f = (double*)a.result + ROVIT_DENSITY_HEADER;
  if (tid < C + 2) {
    long long t = 0;
    for (int w = 0; w < a.chunks; ++w) t += a.ccnt[(size_t)w * (C + 2) + tid];
    s_tot[tid] = t;
  }
  __syncthreads();
  long long n_valid = 0;
  for (int c = 0; c < C; ++c) n_valid += s_tot[c];
  if (tid == 0) {
    head[ROVIT_DENSITY_N] = a.n;
    head[ROVIT_DENSITY_N_VALID] = n_valid;
    head[ROVIT_DENSITY_BAD_LABELS] = s_tot[C];
    head[ROVIT_DENSITY_BAD_ROWS] = s_tot[C + 1];
    for (int c = 0; c < ROVIT_DENSITY_HEADER - ROVIT_DENSITY_COUNTS; ++c) head[ROVIT_DENSITY_COUNTS + c] = c < C ? s_tot[c] : 0;   // and the unused words
  }
  if (tid < E) {
    double g = 0.0;
    for (int c = 0; c < C; ++c) {
      double s = 0.0;
      for (int w = 0; w < a.chunks; ++w) s += a.csum[((size_t)w * C + c) * E + tid];
      const double m = s_tot[c] > 0 ? s / (double)s_tot[c] : 0.0;
      f[(size_t)c * E + tid] = m;
      a.mean32[c * E + tid] = (float)m;
      g += s;
    }
    f[(size_t)C * E + tid] = n_valid > 0 ? g / (double)n_valid : 0.0;
  }
}

struct PlainRow {               // gram_slab's B operand: the row itself, whichever row
  __device__ __forceinline__ PlainRow operator()(int) const { return *this; }
  __device__ __forceinline__ float operator()(float x) const { return x; }
};

template <int T>
__global__ __launch_bounds__(NT) void dens_scatter_kernel(const MomArgs a) {
  constexpr int E = 32 * T, TILES = upper_tiles(T), NQ = (TILES + 3) / 4;
  __shared__ __attribute__((aligned(16))) float Xs[SLAB * E];
  const int tid = threadIdx.x, n = a.n;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  int ti[NQ], tj[NQ];
  wave_tiles<T>(wv, ti, tj);
  for (int w = blockIdx.x; w < a.chunks; w += gridDim.x) {
    f32x16 acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    for (int s0 = 0; s0 < a.R; s0 += SLAB) {
      const int rb = w * a.R + s0;
      if (rb >= n) break;
      __syncthreads();
#pragma unroll
      for (int it = 0; it < T; ++it) {                          // SLAB * E / 4 = 256 T float4
        const int idx = tid + NT * it, row = idx / (E / 4), c4 = idx - row * (E / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const int gr = rb + row;
        const int c = gr < n ? a.cls[gr] : -1;
        if (c >= 0) {
          const float4 xv = *reinterpret_cast<const float4*>(a.x + (size_t)gr * E + 4 * c4);
          const float4 mv = *reinterpret_cast<const float4*>(a.mean32 + c * E + 4 * c4);
          v = make_float4(xv.x - mv.x, xv.y - mv.y, xv.z - mv.z, xv.w - mv.w);
        }
        *reinterpret_cast<float4*>(Xs + row * E + 4 * c4) = v;
      }
      __syncthreads();
      gram_slab<T>(acc, Xs, wv, ti, tj, PlainRow());            // k = the rows of the chunk in order
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (wv + 4 * q < TILES) store_acc_tile(a.part + ((size_t)w * TILES + (wv + 4 * q)) * 1024, acc[q]);
  }
}

__global__ __launch_bounds__(NT) void dens_fold_kernel(const MomArgs a) {
  const int E = a.E, T = E / 32, tiles = upper_tiles(T), items = tiles * 4;
  double* S = (double*)a.result + ROVIT_DENSITY_HEADER + (size_t)(a.C + 1) * E;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int q = w >> 2, el = (w & 3) * NT + threadIdx.x;
    int ra, rb;
    if (fold_element(q, el, T, ra, rb)) continue;               // the diagonal tiles' lower half is the mirror of their upper half
    double s = 0.0;
    for (int c = 0; c < a.chunks; ++c) s += (double)a.part[((size_t)c * tiles + q) * 1024 + el];
    S[(size_t)ra * E + rb] = s;
    S[(size_t)rb * E + ra] = s;
  }
}

// ---- score ---------------------------------------------------------------------------------------------------------------------------

inline size_t score_lds_bytes(int E, int C) { return ((size_t)(SCORE_ROWS + 64) * (E + 4) + (size_t)(C + 1) * E + SCORE_ROWS) * 4; }

__global__ __launch_bounds__(NT) void dens_score_kernel(const rovit_density_scores a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int E = a.embed, C = a.num_classes, B = a.batch, ST = E + 4, T = E / 32, E4 = E / 4;
  float* Fs = lds;                                              // [64][ST] feature rows
  float* Ws = Fs + SCORE_ROWS * ST;                             // [2][32][ST] one row tile of W and of W0
  float* Ms = Ws + 64 * ST;                                     // [C + 1][E] whitened class means, then m0
  float* s_d0 = Ms + (C + 1) * E;                               // [64]
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), mat = wv >> 1, rt = wv & 1;
  const int base = mat ? C : 0, nc = mat ? 1 : C;
  const int tiles = (B + SCORE_ROWS - 1) / SCORE_ROWS;
  for (int k = tid; k < (C + 1) * E; k += NT) Ms[k] = k < C * E ? a.class_means[k] : a.background_mean[k - C * E];
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = tile * SCORE_ROWS;
    __syncthreads();
    for (int idx = tid; idx < SCORE_ROWS * E4; idx += NT) {
      const int row = idx / E4, c4 = idx - row * E4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + row < B) v = *reinterpret_cast<const float4*>(a.features + (size_t)(r0 + row) * E + 4 * c4);
      *reinterpret_cast<float4*>(Fs + row * ST + 4 * c4) = v;
    }
    float p[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) p[c] = 0.f;
    for (int at = 0; at < T; ++at) {
      const int a0 = 32 * at, kend = a0 + 32, k4 = kend / 4;
      __syncthreads();
      for (int idx = tid; idx < 64 * k4; idx += NT) {           // rows a0 .. a0 + 31 of W, then of W0, columns 0 .. a0 + 31
        const int row = idx / k4, c4 = idx - row * k4;
        const float* src = (row < 32 ? a.whitening : a.background_whitening) + (size_t)(a0 + (row & 31)) * E + 4 * c4;
        *reinterpret_cast<float4*>(Ws + row * ST + 4 * c4) = *reinterpret_cast<const float4*>(src);
      }
      __syncthreads();
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* wrow = Ws + (mat * 32 + l31) * ST + 4 * lh;   // A[m = a][k]: plain rows, lane half h holds k = kk + 4h + s in step s
      const float* frow = Fs + (rt * 32 + l31) * ST + 4 * lh;    // B[k][n = row]
      acc = tile_dot(acc, wrow, frow, kend);                       // a run-time bound: the columns up to the diagonal tile
      // lane (l31, h) holds z[row l31][a0 + acc_row(r, h)]
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ai = a0 + acc_row(r, lh);
        const float z = acc[r];
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < nc) {
            const float d = z - Ms[(base + c) * E + ai];
            p[c] = fmaf(d, d, p[c]);
          }
      }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) p[c] += __shfl_xor(p[c], 32);
    if (mat == 1 && lh == 0) s_d0[rt * 32 + l31] = p[0];
    __syncthreads();
    const int row = r0 + rt * 32 + l31;
    if (mat == 0 && lh == 0 && row < B) {
      const float d0 = s_d0[rt * 32 + l31];
      float dmin = p[0], rmin = p[0] - d0;
      int arg = 0;
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < C) {
          a.class_distances[(size_t)row * C + c] = p[c];
          if (c > 0 && p[c] < dmin) { dmin = p[c]; arg = c; }
          if (c > 0) rmin = fminf(rmin, p[c] - d0);
        }
      a.background_distance[row] = d0;
      a.mahalanobis[row] = dmin;
      a.nearest_class[row] = arg;
      a.relative_mahalanobis[row] = rmin;
      if (a.cls_logits) {
        // fp64: energy = -(m + log1p(rest)), max_prob_score = rest / (1 + rest), rest = sum over all but the first maximum of exp(l - m)
        const float* lg = a.cls_logits + (size_t)row * C;
        double m = (double)lg[0];
        int am = 0;
        for (int c = 1; c < C; ++c)
          if ((double)lg[c] > m) { m = (double)lg[c]; am = c; }
        double rest = 0.0;
        for (int c = 0; c < C; ++c)
          if (c != am) rest += exp((double)lg[c] - m);
        a.energy[row] = (float)(-(m + log1p(rest)));
        a.max_prob_score[row] = (float)(rest / (1.0 + rest));
      }
    }
  }
}

// ---- OOD metrics ---------------------------------------------------------------------------------------------------------------------

struct OodLayout { size_t cnt, part, total; };
inline OodLayout ood_layout(int n_in, int n_out) {
  const size_t N = (size_t)n_in + n_out, chunks = (N + NT - 1) / NT;
  OodLayout l;
  l.cnt = 0;
  l.part = l.cnt + rovit_up16(4 * N * 4);
  l.total = l.part + rovit_up16(2 * chunks * 8);
  return l;
}

struct OodArgs {
  int n_in, n_out, N, chunks, L;
  int k[ROVIT_OOD_MAX_LEVELS];
  const float* s_in;
  const float* s_out;
  unsigned* cnt;            // (4, N): less_in, eq_in, less_out, eq_out of every row, the in rows first
  double* part;             // (chunks, 2): the chunk's AP_out and AP_in terms
  void* result;
};

__device__ __forceinline__ float ood_row(const OodArgs& a, int i) { return i < a.n_in ? a.s_in[i] : a.s_out[i - a.n_in]; }

__global__ __launch_bounds__(NT) void ood_rank_kernel(const OodArgs a, int splits, int tiles_per_split) {
  __shared__ __attribute__((aligned(16))) float sX[RANK_RT];
  const int tid = threadIdx.x, N = a.N;
  const int tin = (a.n_in + RANK_RT - 1) / RANK_RT, ntiles = tin + (a.n_out + RANK_RT - 1) / RANK_RT;
  const int items = a.chunks * splits;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int chunk = w % a.chunks, split = w / a.chunks;
    const int i = chunk * NT + tid;
    const float xi = i < N ? ood_row(a, i) : 0.f;
    unsigned less[2] = {0, 0}, eq[2] = {0, 0};
    const int t0 = split * tiles_per_split, t1 = min(ntiles, t0 + tiles_per_split);
    for (int t = t0; t < t1; ++t) {
      const int side = t >= tin, j0 = (side ? t - tin : t) * RANK_RT, lim = side ? a.n_out : a.n_in;
      const float* X = side ? a.s_out : a.s_in;
      __syncthreads();
      rank_stage_tile(sX, X, j0, lim);
      __syncthreads();
      unsigned l = 0, e = 0;
      rank_count_tile(sX, xi, l, e);
      if (side) { less[1] += l; eq[1] += e; } else { less[0] += l; eq[0] += e; }
    }
    if (i < N) {
      atomicAdd(&a.cnt[i], less[0]);
      atomicAdd(&a.cnt[(size_t)N + i], eq[0]);
      atomicAdd(&a.cnt[2 * (size_t)N + i], less[1]);
      atomicAdd(&a.cnt[3 * (size_t)N + i], eq[1]);
    }
  }
}

__global__ __launch_bounds__(NT) void ood_terms_kernel(const OodArgs a) {
  __shared__ double s_d[4];
  __shared__ unsigned long long s_u[4];
  const int tid = threadIdx.x, N = a.N;
  long long* res = (long long*)a.result;
  for (int w = blockIdx.x; w < a.chunks; w += gridDim.x) {
    const int i = w * NT + tid;
    double t_out = 0.0, t_in = 0.0;
    unsigned long long u2 = 0, bad = 0;
    if (i < N) {
      const float x = ood_row(a, i);
      const long long li = a.cnt[i], ei = a.cnt[(size_t)N + i], lo = a.cnt[2 * (size_t)N + i], eo = a.cnt[3 * (size_t)N + i];
      bad = !isfinite(x);
      if (i >= a.n_in) {
        u2 = (unsigned long long)(2 * li + ei);
        const long long ge_out = a.n_out - lo, ge_in = a.n_in - li;
        t_out = ge_out + ge_in > 0 ? (double)ge_out / (double)(ge_out + ge_in) : 0.0;
      } else {
        const long long le_in = li + ei, le_out = lo + eo;
        t_in = le_in + le_out > 0 ? (double)le_in / (double)(le_in + le_out) : 0.0;
        for (int l = 0; l < a.L; ++l)
          if (li < a.k[l] && a.k[l] <= li + ei) {               // every row of the tie group writes the same two words
            ((double*)a.result)[ROVIT_OOD_THRESHOLD + l] = (double)x + 0.0;          // -0 equals +0 and may share the group: +0 is written
            res[ROVIT_OOD_OUT_BELOW + l] = le_out;
          }
      }
    }
    const double so = block_sum_t(t_out, s_d);
    const double si = block_sum_t(t_in, s_d);
    const unsigned long long su = block_sum_t(u2, s_u);
    const unsigned long long sb = block_sum_t(bad, s_u);
    if (tid == 0) {
      a.part[2 * (size_t)w] = so;
      a.part[2 * (size_t)w + 1] = si;
      if (su) atomicAdd((unsigned long long*)&res[ROVIT_OOD_TWO_U], su);
      if (sb) atomicAdd((unsigned long long*)&res[ROVIT_OOD_BAD], sb);
    }
  }
}

__global__ __launch_bounds__(NT) void ood_final_kernel(const OodArgs a) {
  __shared__ double s_d[4];
  const int tid = threadIdx.x;
  double so = 0.0, si = 0.0;
  for (int c = tid; c < a.chunks; c += NT) {
    so += a.part[2 * (size_t)c];
    si += a.part[2 * (size_t)c + 1];
  }
  so = block_sum_t(so, s_d);
  si = block_sum_t(si, s_d);
  if (tid == 0) {
    long long* res = (long long*)a.result;
    res[ROVIT_OOD_N_IN] = a.n_in;
    res[ROVIT_OOD_N_OUT] = a.n_out;
    for (int l = 0; l < a.L; ++l) res[ROVIT_OOD_K + l] = a.k[l];
    ((double*)a.result)[ROVIT_OOD_AP_OUT_SUM] = so;
    ((double*)a.result)[ROVIT_OOD_AP_IN_SUM] = si;
  }
}

inline bool mom_limits_ok(int n, int E, int C) {
  return n >= 1 && n <= ROVIT_KAN_STATS_MAX_ROWS && E >= 32 && E <= 256 && E % 32 == 0 && C >= 2 && C <= MAXC;
}
inline bool ood_limits_ok(int n_in, int n_out) {
  return n_in >= 1 && n_out >= 1 && (long long)n_in + n_out <= ROVIT_EVAL_MAX_ROWS;
}

template <int T>
void launch_scatter(dim3 grid, hipStream_t s, const MomArgs& a) {
  hipLaunchKernelGGL(dens_scatter_kernel<T>, grid, dim3(NT), 0, s, a);
}

}  // namespace

extern "C" size_t rovit_density_workspace_bytes(int n, int E, int C) { return mom_limits_ok(n, E, C) ? mom_layout(n, E, C).total : 0; }

extern "C" int rovit_density_moments(const rovit_density_fit* p, rovit_stream_t stream) {
  const char* who = "density_moments";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_KAN_STATS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_KAN_STATS_MAX_ROWS);
  ROVIT_CHECK_ARG(p->embed >= 32 && p->embed <= 256 && p->embed % 32 == 0, ROVIT_ERR_SHAPE, "%s: embed %d (a multiple of 32 in 32..256)", who,
                  p->embed);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= MAXC, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who, p->num_classes, MAXC);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->features && p->labels && p->workspace && p->result, ROVIT_ERR_NULL, "%s: a null pointer", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->features) && rovit_aligned(p->labels, 4) && rovit_aligned16(p->workspace) && rovit_aligned(p->result, 8),
                  ROVIT_ERR_ALIGN, "%s: the features or the workspace are not 16-byte aligned, or the labels or the result block not to their words", who);
  const int n = p->n, E = p->embed, C = p->num_classes;
  const MomLayout l = mom_layout(n, E, C);
  ROVIT_CHECK_ARG(p->workspace_bytes >= l.total, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes,
                  l.total);
  char* ws = (char*)p->workspace;
  MomArgs a;
  a.n = n; a.E = E; a.C = C; a.R = density_chunk_rows(n); a.chunks = (n + a.R - 1) / a.R;
  a.x = p->features; a.labels = p->labels;
  a.cls = (int*)(ws + l.cls);
  a.csum = (double*)(ws + l.csum);
  a.ccnt = (long long*)(ws + l.ccnt);
  a.mean32 = (float*)(ws + l.mean32);
  a.part = (float*)(ws + l.part);
  a.result = p->result;
  hipStream_t s = (hipStream_t)stream;
  auto grid = [&](long long items) { return rovit_grid(items, p->max_workgroups); };
  hipLaunchKernelGGL(dens_sums_kernel, grid(a.chunks), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("dens_sums_kernel");
  hipLaunchKernelGGL(dens_means_kernel, dim3(1), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("dens_means_kernel");
  switch (E / 32) {
    case 1: launch_scatter<1>(grid(a.chunks), s, a); break;
    case 2: launch_scatter<2>(grid(a.chunks), s, a); break;
    case 3: launch_scatter<3>(grid(a.chunks), s, a); break;
    case 4: launch_scatter<4>(grid(a.chunks), s, a); break;
    case 5: launch_scatter<5>(grid(a.chunks), s, a); break;
    case 6: launch_scatter<6>(grid(a.chunks), s, a); break;
    case 7: launch_scatter<7>(grid(a.chunks), s, a); break;
    default: launch_scatter<8>(grid(a.chunks), s, a); break;
  }
  ROVIT_CHECK_LAUNCH("dens_scatter_kernel");
  hipLaunchKernelGGL(dens_fold_kernel, grid(4ll * upper_tiles(E / 32)), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("dens_fold_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_density_score(const rovit_density_scores* p, rovit_stream_t stream) {
  const char* who = "density_score";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->batch >= 1, ROVIT_ERR_SHAPE, "%s: batch %d (>= 1)", who, p->batch);
  ROVIT_CHECK_ARG(p->embed >= 32 && p->embed <= 256 && p->embed % 32 == 0, ROVIT_ERR_SHAPE, "%s: embed %d (a multiple of 32 in 32..256)", who,
                  p->embed);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= MAXC, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who, p->num_classes, MAXC);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->features && p->whitening && p->class_means && p->background_whitening && p->background_mean, ROVIT_ERR_NULL,
                  "%s: the features or a table are missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->class_distances && p->background_distance && p->mahalanobis && p->nearest_class && p->relative_mahalanobis, ROVIT_ERR_NULL,
                  "%s: an output is missing (null pointer)", who);
  ROVIT_CHECK_ARG(!p->cls_logits || (p->energy && p->max_prob_score), ROVIT_ERR_NULL, "%s: logits without the energy and max_prob_score outputs", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->features) && rovit_aligned16(p->whitening) && rovit_aligned16(p->background_whitening), ROVIT_ERR_ALIGN,
                  "%s: the features or a whitening matrix are not 16-byte aligned", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->class_means, 4) && rovit_aligned(p->background_mean, 4) && rovit_aligned(p->cls_logits, 4) &&
                      rovit_aligned(p->class_distances, 4) && rovit_aligned(p->background_distance, 4) && rovit_aligned(p->mahalanobis, 4) &&
                      rovit_aligned(p->nearest_class, 4) && rovit_aligned(p->relative_mahalanobis, 4) && rovit_aligned(p->energy, 4) &&
                      rovit_aligned(p->max_prob_score, 4),
                  ROVIT_ERR_ALIGN, "%s: an array is not aligned to its element size", who);
  const size_t lds = score_lds_bytes(p->embed, p->num_classes);
  ROVIT_CHECK_ARG(rovit_set_max_lds((const void*)dens_score_kernel, lds), ROVIT_ERR_LAUNCH, "%s: cannot raise the LDS limit", who);
  const long long tiles = ((long long)p->batch + SCORE_ROWS - 1) / SCORE_ROWS;
  hipLaunchKernelGGL(dens_score_kernel, rovit_grid(tiles, p->max_workgroups), dim3(NT), lds, (hipStream_t)stream, *p);
  ROVIT_CHECK_LAUNCH("dens_score_kernel");
  return ROVIT_OK;
}

extern "C" size_t rovit_ood_metrics_workspace_bytes(int n_in, int n_out) { return ood_limits_ok(n_in, n_out) ? ood_layout(n_in, n_out).total : 0; }

namespace {
// the rank workspace of the sorted OOD card: the sorted keys and the permutations of the two populations, then the sort's own
struct OodRankLayout { size_t keys_in, keys_out, perm_in, perm_out, sort, total; };
inline OodRankLayout ood_rank_layout(int n_in, int n_out) {
  const int nn[2] = {n_in, n_out};
  OodRankLayout l;
  l.keys_in = 0;
  l.keys_out = l.keys_in + rovit_up16((size_t)n_in * 4);
  l.perm_in = l.keys_out + rovit_up16((size_t)n_out * 4);
  l.perm_out = l.perm_in + rovit_up16((size_t)n_in * 4);
  l.sort = l.perm_out + rovit_up16((size_t)n_out * 4);
  l.total = l.sort + rovit_sort_batch_workspace_bytes(nn, 2);
  return l;
}
}  // namespace

extern "C" size_t rovit_ood_metrics_rank_workspace_bytes(int n_in, int n_out) {
  return ood_limits_ok(n_in, n_out) ? ood_rank_layout(n_in, n_out).total : 0;
}

extern "C" int rovit_ood_metrics(const rovit_ood* p, rovit_stream_t stream) {
  return rovit_ood_metrics_ex(p, ROVIT_RANK_COUNT, nullptr, 0, stream);
}

extern "C" int rovit_ood_metrics_ex(const rovit_ood* p, int method, void* rank_workspace, size_t rank_workspace_bytes, rovit_stream_t stream) {
  const char* who = "ood_metrics";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(ood_limits_ok(p->n_in, p->n_out), ROVIT_ERR_SHAPE, "%s: %d + %d scores (each >= 1, together at most %d)", who, p->n_in, p->n_out,
                  ROVIT_EVAL_MAX_ROWS);
  ROVIT_CHECK_ARG(p->num_levels >= 0 && p->num_levels <= ROVIT_OOD_MAX_LEVELS, ROVIT_ERR_SHAPE, "%s: %d TPR levels (0..%d)", who, p->num_levels,
                  ROVIT_OOD_MAX_LEVELS);
  for (int l = 0; l < p->num_levels; ++l)
    ROVIT_CHECK_ARG(p->tpr_levels[l] > 0.0 && p->tpr_levels[l] <= 1.0, ROVIT_ERR_SHAPE, "%s: TPR level %d is %g (0 < level <= 1)", who, l,
                    p->tpr_levels[l]);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->scores_in && p->scores_out && p->workspace && p->result, ROVIT_ERR_NULL, "%s: a null pointer", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->scores_in, 4) && rovit_aligned(p->scores_out, 4) && rovit_aligned16(p->workspace) && rovit_aligned(p->result, 8),
                  ROVIT_ERR_ALIGN, "%s: the scores, the workspace or the result block are not aligned", who);
  const OodLayout l = ood_layout(p->n_in, p->n_out);
  ROVIT_CHECK_ARG(p->workspace_bytes >= l.total, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes,
                  l.total);
  ROVIT_CHECK_ARG(method >= ROVIT_RANK_AUTO && method <= ROVIT_RANK_SORT, ROVIT_ERR_SHAPE, "%s: unknown rank method %d", who, method);
  const bool sorted = rovit_rank_method(method, (long long)p->n_in + p->n_out) == ROVIT_RANK_SORT;
  const OodRankLayout rl = ood_rank_layout(p->n_in, p->n_out);
  if (sorted) {
    ROVIT_CHECK_ARG(rank_workspace, ROVIT_ERR_NULL, "%s: the rank workspace is missing (null pointer)", who);
    ROVIT_CHECK_ARG(rovit_aligned16(rank_workspace), ROVIT_ERR_ALIGN, "%s: the rank workspace is not 16-byte aligned", who);
    ROVIT_CHECK_ARG(rank_workspace_bytes >= rl.total, ROVIT_ERR_SHAPE, "%s: the rank workspace holds %zu bytes, %zu are needed", who,
                    rank_workspace_bytes, rl.total);
  }
  char* ws = (char*)p->workspace;
  OodArgs a;
  a.n_in = p->n_in; a.n_out = p->n_out; a.N = p->n_in + p->n_out; a.chunks = (a.N + NT - 1) / NT; a.L = p->num_levels;
  for (int i = 0; i < ROVIT_OOD_MAX_LEVELS; ++i) {
    long long k = i < a.L ? (long long)ceil(p->tpr_levels[i] * (double)p->n_in) : 1;
    a.k[i] = (int)(k < 1 ? 1 : (k > p->n_in ? p->n_in : k));
  }
  a.s_in = p->scores_in; a.s_out = p->scores_out;
  a.cnt = (unsigned*)(ws + l.cnt);
  a.part = (double*)(ws + l.part);
  a.result = p->result;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(a.cnt, 0, l.part - l.cnt, s) != hipSuccess || hipMemsetAsync(p->result, 0, ROVIT_OOD_WORDS * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  auto grid = [&](long long items) { return rovit_grid(items, p->max_workgroups); };
  const int ntiles = (a.n_in + RANK_RT - 1) / RANK_RT + (a.n_out + RANK_RT - 1) / RANK_RT;
  // split the j range until about 1024 workgroups exist; the counts are integers, so the split changes nothing
  int splits = (1024 + a.chunks - 1) / a.chunks;
  splits = splits < 1 ? 1 : (splits > ntiles ? ntiles : splits);
  const int tps = (ntiles + splits - 1) / splits;
  splits = (ntiles + tps - 1) / tps;
  if (sorted) {
    // both populations sorted once; less and eq of every row among the in rows and among the out rows by searches in the two key arrays
    char* rws = (char*)rank_workspace;
    unsigned* k_in = (unsigned*)(rws + rl.keys_in);
    unsigned* k_out = (unsigned*)(rws + rl.keys_out);
    const RovitSortCol c[2] = {{a.s_in, k_in, (unsigned*)(rws + rl.perm_in), a.n_in}, {a.s_out, k_out, (unsigned*)(rws + rl.perm_out), a.n_out}};
    int rc = rovit_sort_batch(c, 2, rws + rl.sort, rank_workspace_bytes - rl.sort, p->max_workgroups, s, who);
    if (rc != ROVIT_OK) return rc;
    const size_t N = (size_t)a.N;
    const RovitRankQuery q[4] = {{a.s_in, a.n_in, k_in, a.n_in, a.cnt, a.cnt + N},
                                 {a.s_out, a.n_out, k_in, a.n_in, a.cnt + a.n_in, a.cnt + N + a.n_in},
                                 {a.s_in, a.n_in, k_out, a.n_out, a.cnt + 2 * N, a.cnt + 3 * N},
                                 {a.s_out, a.n_out, k_out, a.n_out, a.cnt + 2 * N + a.n_in, a.cnt + 3 * N + a.n_in}};
    rc = rovit_rank_search(q, 4, p->max_workgroups, s, who);
    if (rc != ROVIT_OK) return rc;
  } else {
    hipLaunchKernelGGL(ood_rank_kernel, grid((long long)a.chunks * splits), dim3(NT), 0, s, a, splits, tps);
    ROVIT_CHECK_LAUNCH("ood_rank_kernel");
  }
  hipLaunchKernelGGL(ood_terms_kernel, grid(a.chunks), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("ood_terms_kernel");
  hipLaunchKernelGGL(ood_final_kernel, dim3(1), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("ood_final_kernel");
  return ROVIT_OK;
}
