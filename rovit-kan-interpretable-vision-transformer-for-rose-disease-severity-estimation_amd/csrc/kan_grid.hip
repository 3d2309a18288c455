// KAN grid extension: refit every edge spline of one layer to a new uniform knot vector by least squares on data
// (rovit_kan_regrid_moments, rovit_kan_regrid_solve).  Definitions: DESIGN.md section 2 and include/rovit_hip.h.
//
// Reference being extended: models/kan.py:8-44 fixes the knots at construction; nothing there moves a trained edge function to another
// grid.  pykan calls the operation update_grid_from_samples / refine.
//
// For input i of the layer, with b the old basis and b' the new one, both of v = tanh(x_ni) and both from kan_basis (kan_device.h):
//   G_i = sum_n b' b'^T (4 diagonals)    M_i = sum_n b' b^T (one 4 x 4 block per row)    O_i = sum_n b b^T (4 diagonals)
// over the finite rows.  A row lies in ONE knot interval j' of the new grid and ONE interval j of the old one, and both are monotone in
// v, so the pairs (j', j) that occur lie on a monotone staircase and j' + j names a pair uniquely: the moments are first accumulated
// per CELL -- G per j', O per j, M per j' + j, 16 products each -- and then gathered into the banded / dense result.
//
//   regrid_cells_kernel   a workgroup owns one input and a fixed range of 256-row chunks.  Per chunk every (row, input) gets tanhf and the
//                         two bases ONCE into LDS.  Wave 0 owns the G cells, wave 1 the O cells, waves 2-3 the M cells, one cell per thread:
//                         the owner walks the staged rows in row order, adds the 16 products of the rows that fall into its cell in fp32
//                         over 16 staged rows at a time and folds them into fp64.  Finite rows and non-finite inputs: integer atomics.
//   regrid_fold_kernel    a workgroup per input: thread 0 walks the merged knots once to name the pair of every M cell, then every entry
//                         of G, M, O adds its cells in cell order and, inside a cell, the row ranges in range order.
//   regrid_solve_kernel   a workgroup per input, fp64 in LDS: A = G_i / N_i + prior_g (+ delta on unreached diagonal entries), Cholesky, T = A^-1 (M_i / N_i + prior_m),
//                         then one wave per output: c' = T c, the fit and target mean squares.
// Every partition is a function of n and the shapes only and every floating sum has a fixed order: the results are bit-identical from
// run to run.  No (n, in, nb) tensor exists.
#include "kan_device.h"

namespace {

constexpr int NT = 256;                 // threads per workgroup
constexpr int SR = 256;                 // rows per chunk: one per thread when staging
constexpr int FOLD = 16;                // staged rows summed in fp32 before the fold into fp64
constexpr int MAX_SPLITS = 64;          // row ranges at most
constexpr int WANT_WG = 1024;           // workgroups aimed at: four per CU
constexpr int MIN_KNOTS = 8;

static bool shape_ok(int in_f, int out_f, int nko, int nkn) {
  return in_f >= 1 && out_f >= 1 && nko >= MIN_KNOTS && nko <= KAN_MAX_KNOTS && nkn >= MIN_KNOTS && nkn <= KAN_MAX_KNOTS;
}

struct Geometry {
  int chunks, splits, chunks_per_split;
  int cells;             // nb' + nb + (nb' + nb - 1)
};

static Geometry geometry(int n, int in_f, int nko, int nkn) {
  Geometry g;
  g.chunks = (n + SR - 1) / SR;
  int s = (WANT_WG + in_f - 1) / in_f;
  s = s < 1 ? 1 : (s > MAX_SPLITS ? MAX_SPLITS : s);
  s = s > g.chunks ? g.chunks : s;
  g.chunks_per_split = (g.chunks + s - 1) / s;
  g.splits = (g.chunks + g.chunks_per_split - 1) / g.chunks_per_split;
  g.cells = 2 * (nkn - 4) + 2 * (nko - 4) - 1;
  return g;
}

__global__ __launch_bounds__(NT) void regrid_cells_kernel(const rovit_kan_regrid a, int chunks_per_split, int cells, double* __restrict__ part,
                                                          unsigned long long* __restrict__ counts) {
  __shared__ float s_ko[KAN_MAX_KNOTS], s_kn[KAN_MAX_KNOTS];
  __shared__ int s_key[3][SR];                 // the row's cell per role: j', j, j' + j (-1: none)
  __shared__ float s_vn[SR][4], s_vo[SR][4];
  const int tid = threadIdx.x, i = blockIdx.x;
  const int nko = a.n_knots_old, nkn = a.n_knots_new, nb = nko - 4, nbn = nkn - 4;
  if (tid < nko) s_ko[tid] = a.knots_old[tid];
  if (tid < nkn) s_kn[tid] = a.knots_new[tid];
  __syncthreads();
  const float inv_ho = 1.f / (s_ko[1] - s_ko[0]), inv_hn = 1.f / (s_kn[1] - s_kn[0]);
  // role of this thread's wave and its cell
  const int role = tid < 64 ? 0 : (tid < 128 ? 1 : 2);
  const int cell = role == 0 ? tid : (role == 1 ? tid - 64 : tid - 128);
  const bool owner = cell < (role == 0 ? nbn : (role == 1 ? nb : nbn + nb - 1));
  const float(*va)[4] = role == 1 ? s_vo : s_vn;
  const float(*vb)[4] = role == 0 ? s_vn : s_vo;
  double acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0;
  unsigned good = 0, bad = 0;
  const int c0 = blockIdx.y * chunks_per_split;
  const long row_end = min((long)a.n, (long)(c0 + chunks_per_split) * SR);
  for (long row0 = (long)c0 * SR; row0 < row_end; row0 += SR) {
    __syncthreads();
    {
      const long row = row0 + tid;
      int jn = -1, jo = -1;
      float vn[4] = {0.f, 0.f, 0.f, 0.f}, vo[4] = {0.f, 0.f, 0.f, 0.f};
      if (row < row_end) {
        const float x = a.x[(size_t)row * a.in_f + i];
        if (isfinite(x)) {
          const float v = tanhf(x);
          const Basis4 bn = kan_basis<false>(v, s_kn, nkn, inv_hn, nullptr);
          const Basis4 bo = kan_basis<false>(v, s_ko, nko, inv_ho, nullptr);
          jn = bn.j;
          jo = bo.j;
#pragma unroll
          for (int m = 0; m < 4; ++m) { vn[m] = bn.v[m]; vo[m] = bo.v[m]; }
          ++good;
        } else {
          ++bad;
        }
      }
      s_key[0][tid] = jn;
      s_key[1][tid] = jo;
      s_key[2][tid] = (jn >= 0 && jo >= 0) ? jn + jo : -1;
#pragma unroll
      for (int m = 0; m < 4; ++m) { s_vn[tid][m] = vn[m]; s_vo[tid][m] = vo[m]; }
    }
    __syncthreads();
    if (owner) {
      const int rows = (int)min((long)SR, row_end - row0);
      for (int r0 = 0; r0 < rows; r0 += FOLD) {
        float f[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) f[q] = 0.f;
        bool hit = false;
        const int r1 = min(r0 + FOLD, rows);
        for (int r = r0; r < r1; ++r) {
          if (s_key[role][r] != cell) continue;
          hit = true;
#pragma unroll
          for (int m1 = 0; m1 < 4; ++m1)
#pragma unroll
            for (int m2 = 0; m2 < 4; ++m2) f[m1 * 4 + m2] = fmaf(va[r][m1], vb[r][m2], f[m1 * 4 + m2]);
        }
        if (hit) {
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[q] += (double)f[q];
        }
      }
    }
  }
  if (owner) {
    const int slot = role == 0 ? cell : (role == 1 ? nbn + cell : nbn + nb + cell);
    double* dst = part + (((size_t)blockIdx.y * a.in_f + i) * cells + slot) * 16;
#pragma unroll
    for (int q = 0; q < 16; ++q) dst[q] = acc[q];
  }
  // finite rows and non-finite inputs of this range: wave sums, then one integer atomic each
  for (int off = 32; off > 0; off >>= 1) {
    good += __shfl_xor(good, off);
    bad += __shfl_xor(bad, off);
  }
  if ((tid & 63) == 0) {
    if (good) atomicAdd(&counts[i], (unsigned long long)good);
    if (bad) atomicAdd(&counts[a.in_f + i], (unsigned long long)bad);
  }
}

__global__ __launch_bounds__(NT) void regrid_fold_kernel(const rovit_kan_regrid a, int splits, int cells, const double* __restrict__ part) {
  __shared__ int s_tag[2 * KAN_MAX_KNOTS];       // j' of the M cell j' + j; -1: no row can fall there
  const int tid = threadIdx.x, i = blockIdx.x;
  const int nko = a.n_knots_old, nkn = a.n_knots_new, nb = nko - 4, nbn = nkn - 4;
  if (tid < 2 * KAN_MAX_KNOTS) s_tag[tid] = -1;
  __syncthreads();
  if (tid == 0) {
    // the pairs of intervals in ascending v: both searches clamp to their grid first, so below both second knots the pair is (0, 0)
    int jn = 0, jo = 0;
    for (;;) {
      if (jn < nbn && jo < nb) s_tag[jn + jo] = jn;
      const bool en = jn >= nkn - 1, eo = jo >= nko - 1;
      if (en && eo) break;
      const float tn = en ? INFINITY : a.knots_new[jn + 1], to = eo ? INFINITY : a.knots_old[jo + 1];
      const float t = fminf(tn, to);
      if (tn == t) ++jn;
      if (to == t) ++jo;
    }
  }
  __syncthreads();
  const size_t stride = (size_t)a.in_f * cells * 16;                   // one row range of partials
  const double* p0 = part + (size_t)i * cells * 16;
  double* res = reinterpret_cast<double*>(a.moments);
  double* G = res + (size_t)i * nbn * 4;
  double* M = res + (size_t)a.in_f * nbn * 4 + (size_t)i * nbn * nb;
  double* O = res + (size_t)a.in_f * nbn * 4 + (size_t)a.in_f * nbn * nb + (size_t)i * nb * 4;
  const int total = nbn * 4 + nb * 4 + nbn * nb;
  for (int w = tid; w < total; w += NT) {
    double s = 0.0;
    if (w < nbn * 4 + nb * 4) {                                        // band entry [e][d] = sum_n b_e b_(e-d)
      const bool isG = w < nbn * 4;
      const int u = isG ? w : w - nbn * 4, e = u >> 2, d = u & 3, lim = isG ? nbn : nb, base = isG ? 0 : nbn;
      if (e - d >= 0)
        for (int m1 = 0; m1 + d < 4; ++m1) {
          const int c = e + m1;                                        // interval whose basis e is its value m1
          if (c >= lim) break;
          const double* p = p0 + (size_t)(base + c) * 16 + m1 * 4 + m1 + d;
          for (int k = 0; k < splits; ++k) s += p[(size_t)k * stride];
        }
      (isG ? G : O)[u] = s;
    } else {
      const int u = w - nbn * 4 - nb * 4, e = u / nb, b = u % nb;
      for (int c = 0; c < nbn + nb - 1; ++c) {
        const int jn = s_tag[c];
        if (jn < 0) continue;
        const int m1 = jn - e, m2 = c - jn - b;
        if (m1 < 0 || m1 > 3 || m2 < 0 || m2 > 3) continue;
        const double* p = p0 + (size_t)(nbn + nb + c) * 16 + m1 * 4 + m2;
        for (int k = 0; k < splits; ++k) s += p[(size_t)k * stride];
      }
      M[u] = s;
    }
  }
}

__device__ __forceinline__ double wave_sum(double v) {                 // a fixed tree: the same bits every run
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(NT) void regrid_solve_kernel(const rovit_kan_regrid_fit a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, i = blockIdx.x;
  const int nb = a.n_knots_old - 4, nbn = a.n_knots_new - 4;
  double* A = reinterpret_cast<double*>(smem);                          // (nbn, nbn): G_i, then its Cholesky factor (lower)
  double* B = A + nbn * nbn;                                            // (nbn, nb): M_i, then T_i
  double* cw = B + nbn * nb;                                            // (4, 64): the old coefficients of a wave's edge
  __shared__ double s_piv[2];
  __shared__ int s_bad;
  const double* res = reinterpret_cast<const double*>(a.moments);
  const double* Gd = res + (size_t)i * nbn * 4;
  const double* Md = res + (size_t)a.in_f * nbn * 4 + (size_t)i * nbn * nb;
  const double* Od = res + (size_t)a.in_f * nbn * 4 + (size_t)a.in_f * nbn * nb + (size_t)i * nb * 4;
  const long long* cnt = reinterpret_cast<const long long*>(res + (size_t)a.in_f * (nbn * 4 + nbn * nb + nb * 4));
  const long long rows = cnt[i];
  const double inv = rows > 0 ? 1.0 / (double)rows : 0.0;
  for (int w = tid; w < nbn * nbn; w += NT) {
    const int r = w / nbn, c = w % nbn, hi = r > c ? r : c, d = r > c ? r - c : c - r;
    A[w] = a.prior_g[w] + (d < 4 ? Gd[hi * 4 + d] * inv : 0.0);
  }
  for (int w = tid; w < nbn * nb; w += NT) B[w] = a.prior_m[w] + Md[w] * inv;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  if (tid == 0) {
    double tr = 0.0;
    for (int k = 0; k < nbn; ++k) tr += A[k * nbn + k];
    const double delta = 0x1p-40 * tr / nbn;
    for (int k = 0; k < nbn; ++k)                                       // only the bases neither the data nor D reach: see the header
      if (A[k * nbn + k] <= delta) A[k * nbn + k] += delta;
  }
  __syncthreads();
  for (int k = 0; k < nbn; ++k) {
    if (tid == 0) {
      const double p = A[k * nbn + k];
      if (k == 0) s_piv[0] = s_piv[1] = p;
      s_piv[0] = p < s_piv[0] ? p : s_piv[0];
      s_piv[1] = p > s_piv[1] ? p : s_piv[1];
      if (!(p > 0.0)) s_bad = 1;
      else A[k * nbn + k] = sqrt(p);
    }
    __syncthreads();
    if (s_bad) break;
    const double lkk = A[k * nbn + k];
    for (int r = k + 1 + tid; r < nbn; r += NT) A[r * nbn + k] /= lkk;
    __syncthreads();
    const int m = nbn - k - 1;
    for (int w = tid; w < m * m; w += NT) {
      const int r = k + 1 + w / m, c = k + 1 + w % m;
      if (c <= r) A[r * nbn + c] -= A[r * nbn + k] * A[c * nbn + k];
    }
    __syncthreads();
  }
  const bool bad = s_bad != 0;
  if (!bad && tid < nb) {                                               // L y = m, L^T t = y for column tid
    for (int r = 0; r < nbn; ++r) {
      double s = B[r * nb + tid];
      for (int c = 0; c < r; ++c) s -= A[r * nbn + c] * B[c * nb + tid];
      B[r * nb + tid] = s / A[r * nbn + r];
    }
    for (int r = nbn - 1; r >= 0; --r) {
      double s = B[r * nb + tid];
      for (int c = r + 1; c < nbn; ++c) s -= A[c * nbn + r] * B[c * nb + tid];
      B[r * nb + tid] = s / A[r * nbn + r];
    }
  }
  __syncthreads();
  double* diag = reinterpret_cast<double*>(a.diagnostics);
  const size_t E = (size_t)a.in_f * a.out_f;
  if (tid == 0) {
    diag[2 * E + i] = bad ? 0.0 : s_piv[0] / s_piv[1];
    long long* di = reinterpret_cast<long long*>(diag + 2 * E + a.in_f);
    di[i] = rows;
    di[a.in_f + i] = cnt[a.in_f + i];
    if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(di + 2 * a.in_f), 1ull);
  }
  const int lane = tid & 63, wv = tid >> 6;
  double* c = cw + wv * 64;
  for (int j0 = 0; j0 < a.out_f; j0 += NT / 64) {                      // one edge per wave; the trip count is the workgroup's
    const int j = j0 + wv;
    const size_t e = (size_t)i * a.out_f + (j < a.out_f ? j : 0);
    __syncthreads();
    c[lane] = (lane < nb && j < a.out_f) ? (double)a.spline_w[e * nb + lane] : 0.0;
    __syncthreads();
    if (j >= a.out_f) continue;
    double cn = 0.0, mc = 0.0;                                          // c'_lane and (M_d c)_lane
    if (lane < nbn && !bad)
      for (int b = 0; b < nb; ++b) {
        cn = fma(B[lane * nb + b], c[b], cn);
        mc = fma(Md[lane * nb + b] * inv, c[b], mc);
      }
    if (lane < nbn) a.spline_w_new[e * nbn + lane] = (float)cn;
    double qg = 0.0, qo = 0.0;                                          // lane's share of c'^T G_d c' and c^T O c
    const double cl = c[lane];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const double cnd = __shfl_up(cn, d), cld = lane >= d ? c[lane - d] : 0.0;
      if (lane < nbn && lane >= d) qg += (d ? 2.0 : 1.0) * Gd[lane * 4 + d] * inv * cn * cnd;
      if (lane < nb && lane >= d) qo += (d ? 2.0 : 1.0) * Od[lane * 4 + d] * inv * cl * cld;
    }
    const double tg = wave_sum(qg), tm = wave_sum(cn * mc), to = wave_sum(qo);
    if (lane == 0) {
      diag[e] = tg - 2.0 * tm + to;
      diag[E + e] = to;
    }
  }
}

static size_t solve_lds(int nb, int nbn) { return ((size_t)nbn * nbn + (size_t)nbn * nb + 4 * 64) * 8; }

}  // namespace

extern "C" size_t rovit_kan_regrid_moment_words(int in_f, int n_knots_old, int n_knots_new) {
  if (!shape_ok(in_f, 1, n_knots_old, n_knots_new)) return 0;
  const size_t nb = n_knots_old - 4, nbn = n_knots_new - 4;
  return (size_t)in_f * (4 * nbn + nbn * nb + 4 * nb + 2);
}

extern "C" size_t rovit_kan_regrid_diag_words(int in_f, int out_f) {
  if (in_f < 1 || out_f < 1) return 0;
  return 2 * (size_t)in_f * out_f + 3 * (size_t)in_f + 1;
}

extern "C" size_t rovit_kan_regrid_workspace_bytes(int n, int in_f, int n_knots_old, int n_knots_new) {
  if (!shape_ok(in_f, 1, n_knots_old, n_knots_new) || n < 1 || n > ROVIT_KAN_STATS_MAX_ROWS) return 0;
  const Geometry g = geometry(n, in_f, n_knots_old, n_knots_new);
  return (size_t)g.splits * in_f * g.cells * 16 * sizeof(double);
}

extern "C" int rovit_kan_regrid_moments(const rovit_kan_regrid* p, rovit_stream_t stream) {
  const char* who = "kan_regrid_moments";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(shape_ok(p->in_f, 1, p->n_knots_old, p->n_knots_new), ROVIT_ERR_SHAPE, "%s: %d inputs, %d -> %d knots (in >= 1; knots %d..%d)", who,
                  p->in_f, p->n_knots_old, p->n_knots_new, MIN_KNOTS, KAN_MAX_KNOTS);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_KAN_STATS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_KAN_STATS_MAX_ROWS);
  ROVIT_CHECK_ARG(p->x && p->knots_old && p->knots_new, ROVIT_ERR_NULL, "%s: the rows or a knot vector is missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->workspace && p->moments, ROVIT_ERR_NULL, "%s: the workspace or the moment block is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->x, 4) && rovit_aligned(p->knots_old, 4) && rovit_aligned(p->knots_new, 4) && rovit_aligned(p->workspace, 8) &&
                      rovit_aligned(p->moments, 8),
                  ROVIT_ERR_ALIGN, "%s: a pointer is not aligned to its element size", who);
  const size_t need = rovit_kan_regrid_workspace_bytes(p->n, p->in_f, p->n_knots_old, p->n_knots_new);
  ROVIT_CHECK_ARG(p->workspace_bytes >= need, ROVIT_ERR_SHAPE, "%s: workspace of %zu bytes, %zu needed", who, p->workspace_bytes, need);
  const Geometry g = geometry(p->n, p->in_f, p->n_knots_old, p->n_knots_new);
  hipStream_t s = (hipStream_t)stream;
  const size_t nb = p->n_knots_old - 4, nbn = p->n_knots_new - 4;
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(p->moments) + (size_t)p->in_f * (4 * nbn + nbn * nb + 4 * nb);
  if (hipMemsetAsync(counts, 0, (size_t)p->in_f * 2 * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(regrid_cells_kernel, dim3(p->in_f, g.splits), dim3(NT), 0, s, *p, g.chunks_per_split, g.cells,
                     reinterpret_cast<double*>(p->workspace), counts);
  ROVIT_CHECK_LAUNCH("regrid_cells_kernel");
  hipLaunchKernelGGL(regrid_fold_kernel, dim3(p->in_f), dim3(NT), 0, s, *p, g.splits, g.cells, reinterpret_cast<const double*>(p->workspace));
  ROVIT_CHECK_LAUNCH("regrid_fold_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_kan_regrid_solve(const rovit_kan_regrid_fit* p, rovit_stream_t stream) {
  const char* who = "kan_regrid_solve";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(shape_ok(p->in_f, p->out_f, p->n_knots_old, p->n_knots_new), ROVIT_ERR_SHAPE,
                  "%s: layer %d -> %d, %d -> %d knots (in, out >= 1; knots %d..%d)", who, p->in_f, p->out_f, p->n_knots_old, p->n_knots_new, MIN_KNOTS,
                  KAN_MAX_KNOTS);
  ROVIT_CHECK_ARG(p->moments && p->prior_g && p->prior_m && p->spline_w, ROVIT_ERR_NULL, "%s: the moments, a prior or the coefficients are missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->spline_w_new && p->diagnostics, ROVIT_ERR_NULL, "%s: the new coefficients or the diagnostics block is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->moments, 8) && rovit_aligned(p->prior_g, 8) && rovit_aligned(p->prior_m, 8) && rovit_aligned(p->spline_w, 4) &&
                      rovit_aligned(p->spline_w_new, 4) && rovit_aligned(p->diagnostics, 8),
                  ROVIT_ERR_ALIGN, "%s: a pointer is not aligned to its element size", who);
  hipStream_t s = (hipStream_t)stream;
  double* diag = reinterpret_cast<double*>(p->diagnostics);
  if (hipMemsetAsync(diag + 2 * (size_t)p->in_f * p->out_f + 3 * (size_t)p->in_f, 0, 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(regrid_solve_kernel, dim3(p->in_f), dim3(NT), solve_lds(p->n_knots_old - 4, p->n_knots_new - 4), s, *p);
  ROVIT_CHECK_LAUNCH("regrid_solve_kernel");
  return ROVIT_OK;
}
