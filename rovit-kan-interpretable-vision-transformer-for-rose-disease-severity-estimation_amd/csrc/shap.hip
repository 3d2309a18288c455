// KernelSHAP over groups of patches: the coalitions and their src rows, the Gram matrix with its Cholesky factor, and the constrained
// weighted least-squares fit (rovit_shap_coalitions, rovit_shap_gram, rovit_shap_solve).  Definitions: DESIGN.md section 2 and
// include/rovit_hip.h; the host plan and the numpy fp64 reference: rovit_hip/shap.py.
//
//   shap_coalitions_kernel  a workgroup per pair (sample 2k and its complement 2k + 1).  An enumerated pair is unranked by thread 0 with
//                           exact 64-bit binomials; a sampled pair draws one Philox word per player, stages the 64-bit keys
//                           (word << 32) | i in LDS and every player counts the keys below its own: integer compares alone decide
//                           membership.  Then seven threads pack the bits, and a thread per patch writes the 'replace' row and, from the
//                           count of kept patches in front of it, its slot of the 'drop' sequence.
//   shap_gram_kernel        a thread per element of the lower triangle: A[i][j] = sum_m w_m z_mi z_mj over m ascending, the samples staged
//                           in LDS 512 at a time; written to [i][j] and [j][i], and into the factor block.
//   shap_chol_kernel        ONE workgroup of 1024 threads: right-looking Cholesky in fp64, in place in the factor block in GLOBAL memory
//                           (307 KB at P = 196: read through L2; the packed triangle would fill 154 448 B of the 160 KB LDS and leave no
//                           room beside it, and the whole factorisation is 2.5 MFLOP once per call), the current column staged in LDS;
//                           then u = A^-1 1, 1^T u, the smallest pivot and the sum of the weights.
//   shap_solve_kernel       a workgroup per (image, target): b in fp64 over m ascending (the product w_m y_m rounded, then added: the
//                           reference's own order), the two triangular solves against L, lambda, phi, the residual RMS, the patch map.
// Every thread's sum has a fixed order and no partition depends on the grid: all outputs are bit-identical from run to run and for
// every max_workgroups.  No floating-point atomic.  Nothing here is on the matrix cores.
#include "common.h"
#include "philox.h"

namespace {

constexpr int NT = 256;                 // threads per workgroup (>= ROVIT_SHAP_PATCHES: a thread per player / per patch)
constexpr int NT_CHOL = 1024;
constexpr int NP = ROVIT_SHAP_PATCHES;
constexpr int NWORDS = ROVIT_SHAP_WORDS;
constexpr int CH = 512;                 // samples staged in LDS at a time
static_assert(NT >= NP && NWORDS * 32 >= NP, "a thread per patch, a bit per player");

static bool sizes_ok(int P, int M) { return P >= 2 && P <= NP && M >= 1 && M <= ROVIT_SHAP_MAX_SAMPLES; }

static int capped(long long items, int cap) {
  long long g = items < 1 ? 1 : items;
  if (cap > 0 && g > cap) g = cap;
  return (int)g;
}

// C(n, k), exact: after step i the value is C(n - k + i, i).  The host enumerates a class only when all of it fits the budget, so every
// binomial met is at most 2 ROVIT_SHAP_MAX_SAMPLES and the product below stays far inside 64 bits.
__device__ unsigned long long binom(int n, int k) {
  if (k < 0 || k > n) return 0ull;
  if (k > n - k) k = n - k;
  unsigned long long c = 1ull;
  for (int i = 1; i <= k; ++i) c = c * (unsigned long long)(n - k + i) / (unsigned long long)i;
  return c;
}

__global__ __launch_bounds__(NT) void shap_coalitions_kernel(const rovit_shap_coalition_args a) {
  __shared__ unsigned long long s_key[NT];
  __shared__ int s_in[NT];              // player i is in the coalition
  __shared__ int s_keep[NT];            // patch p is kept by the coalition
  const int tid = threadIdx.x, P = a.num_players, pairs = a.num_samples / 2;
  for (int k = blockIdx.x; k < pairs; k += gridDim.x) {
    __syncthreads();                    // the previous pair's readers
    int s = a.pairs[4 * k];
    s = s < 1 ? 1 : (s > P - 1 ? P - 1 : s);
    const int enumerated = a.pairs[4 * k + 1], rank = a.pairs[4 * k + 2];
    if (enumerated) {
      s_in[tid] = 0;
      __syncthreads();
      if (tid == 0) {
        unsigned long long rem = rank < 0 ? 0ull : (unsigned long long)rank;
        int x = 0;
        for (int pos = 0; pos < s && x < P; ++pos)
          for (; x < P; ++x) {          // subsets that put x at this position: C(P - 1 - x, s - 1 - pos)
            const unsigned long long c = binom(P - 1 - x, s - 1 - pos);
            if (rem < c) {
              s_in[x++] = 1;
              break;
            }
            rem -= c;
          }
      }
    } else {
      unsigned long long key = ~0ull;
      if (tid < P) {
        const U4 w4 = philox4x32_10(a.seed, (unsigned)(tid >> 2), (unsigned)rank, ROVIT_SHAP_STREAM, 0u);
        const int q = tid & 3;
        const unsigned w = q == 0 ? w4.x : (q == 1 ? w4.y : (q == 2 ? w4.z : w4.w));
        key = ((unsigned long long)w << 32) | (unsigned long long)tid;
      }
      s_key[tid] = key;
      __syncthreads();
      int below = 0;
      for (int j = 0; j < P; ++j) below += s_key[j] < key;
      s_in[tid] = (tid < P && below < s) ? 1 : 0;
    }
    __syncthreads();
    if (tid < NWORDS) {
      unsigned word = 0u;
      for (int i = 0; i < 32; ++i) {
        const int idx = 32 * tid + i;
        if (idx < P && s_in[idx]) word |= 1u << i;
      }
      const int nb = P - 32 * tid;
      const unsigned valid = nb >= 32 ? ~0u : (nb <= 0 ? 0u : (1u << nb) - 1u);
      a.bits[(size_t)(2 * k) * NWORDS + tid] = word;
      a.bits[(size_t)(2 * k + 1) * NWORDS + tid] = ~word & valid;
    }
    if (tid == 0) {
      const double w = a.pair_weights[k];
      a.weights[2 * k] = w;
      a.weights[2 * k + 1] = w;
    }
    if (a.players) {                    // uniform
      int in = 0;
      if (tid < NP) {
        const int pl = a.players[tid];
        in = (pl >= 0 && pl < P) ? s_in[pl] : 0;
      }
      s_keep[tid] = in;
      __syncthreads();
      if (tid < NP) {
        int before = 0;                 // kept patches of the coalition in front of this one
        for (int q = 0; q < tid; ++q) before += s_keep[q];
        if (a.src_replace) {
          int* r0 = a.src_replace + (size_t)(2 * k) * (NP + 1);
          int* r1 = r0 + (NP + 1);
          r0[1 + tid] = in ? 1 + tid : -2 - tid;
          r1[1 + tid] = in ? -2 - tid : 1 + tid;
          if (tid == 0) r0[0] = r1[0] = 0;
        }
        if (a.src_drop) {
          const long long o0 = a.drop_offsets[2 * k], o1 = a.drop_offsets[2 * k + 1];
          const long long at = in ? o0 + 1 + before : o1 + 1 + (tid - before);
          if (at >= 0 && at < a.drop_words) a.src_drop[at] = 1 + tid;
          if (tid == 0) {
            if (o0 >= 0 && o0 < a.drop_words) a.src_drop[o0] = 0;
            if (o1 >= 0 && o1 < a.drop_words) a.src_drop[o1] = 0;
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(NT) void shap_gram_kernel(const rovit_shap_gram_args a, int items) {
  __shared__ unsigned s_bits[CH * NWORDS];
  __shared__ double s_w[CH];
  const int tid = threadIdx.x, P = a.num_players, M = a.num_samples;
  const int E = P * (P + 1) / 2;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int e = item * NT + tid;
    int i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while (i > 0 && i * (i + 1) / 2 > e) --i;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    const int j = e - i * (i + 1) / 2;
    const bool live = e < E;
    const int wi = (i >> 5) < NWORDS ? (i >> 5) : 0, wj = j >> 5;
    const unsigned bi = 1u << (i & 31), bj = 1u << (j & 31);
    double acc = 0.0;
    for (int m0 = 0; m0 < M; m0 += CH) {
      const int n = min(CH, M - m0);
      __syncthreads();
      for (int q = tid; q < n * NWORDS; q += NT) s_bits[q] = a.bits[(size_t)m0 * NWORDS + q];
      for (int q = tid; q < n; q += NT) s_w[q] = a.weights[m0 + q];
      __syncthreads();
      if (live)
        for (int m = 0; m < n; ++m)
          if ((s_bits[m * NWORDS + wi] & bi) && (s_bits[m * NWORDS + wj] & bj)) acc = __dadd_rn(acc, s_w[m]);
    }
    if (live) {
      a.gram[(size_t)i * P + j] = acc;
      a.gram[(size_t)j * P + i] = acc;
      a.factor[(size_t)i * P + j] = acc;
      if (i != j) a.factor[(size_t)j * P + i] = 0.0;
    }
  }
}

// L is written by some threads and read by others of the SAME workgroup across __syncthreads(), which orders global memory at workgroup
// scope; the pointer is deliberately neither const nor __restrict__.
__global__ __launch_bounds__(NT_CHOL) void shap_chol_kernel(double* f, int P, const double* weights, int M) {
  __shared__ double s_col[NP], s_u[NP], s_red[NT_CHOL / 64];
  __shared__ double s_piv;
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  double* L = f;
  if (tid == 0) {
    s_bad = 0;
    s_piv = INFINITY;
  }
  __syncthreads();
  for (int k = 0; k < P; ++k) {
    if (tid == 0) {
      const double p = L[(size_t)k * P + k];
      if (!(p >= s_piv)) s_piv = p;                       // the smallest pivot; a NaN pivot is kept
      if (!(p > 0.0)) s_bad = 1;
      else L[(size_t)k * P + k] = sqrt(p);
    }
    __syncthreads();
    if (s_bad) break;                                     // uniform
    const double lkk = L[(size_t)k * P + k];
    for (int r = k + 1 + tid; r < P; r += NT_CHOL) {
      const double v = L[(size_t)r * P + k] / lkk;
      L[(size_t)r * P + k] = v;
      s_col[r] = v;
    }
    __syncthreads();
    const int m = P - k - 1;
    for (int w = tid; w < m * m; w += NT_CHOL) {
      const int r = k + 1 + w / m, c = k + 1 + w % m;
      if (c <= r) L[(size_t)r * P + c] -= s_col[r] * s_col[c];
    }
    __syncthreads();
  }
  const bool bad = s_bad != 0;
  if (tid < P) s_u[tid] = bad ? __builtin_nan("") : 1.0;
  __syncthreads();
  if (!bad) {
    for (int k = 0; k < P; ++k) {                         // L y = 1
      if (tid == 0) s_u[k] /= L[(size_t)k * P + k];
      __syncthreads();
      const double yk = s_u[k];
      for (int r = k + 1 + tid; r < P; r += NT_CHOL) s_u[r] -= L[(size_t)r * P + k] * yk;
      __syncthreads();
    }
    for (int k = P - 1; k >= 0; --k) {                    // L^T u = y
      if (tid == 0) s_u[k] /= L[(size_t)k * P + k];
      __syncthreads();
      const double uk = s_u[k];
      for (int r = tid; r < k; r += NT_CHOL) s_u[r] -= L[(size_t)k * P + r] * uk;
      __syncthreads();
    }
  }
  double part = 0.0;                                      // the sum of the weights: a thread's share in m order, then the fixed tree
  for (int m = tid; m < M; m += NT_CHOL) part += weights[m];
  const double sum_w = block_sum_t<NT_CHOL / 64>(part, s_red);
  double* tail = f + (size_t)P * P;
  if (tid < P) tail[tid] = s_u[tid];
  if (tid == 0) {
    double su = 0.0;
    for (int i = 0; i < P; ++i) su += s_u[i];
    tail[P] = su;
    tail[P + 1] = s_piv;
    tail[P + 2] = bad ? 0.0 : 1.0;
    tail[P + 3] = sum_w;
  }
}

__global__ __launch_bounds__(NT) void shap_solve_kernel(const rovit_shap_solve_args a) {
  __shared__ unsigned s_bits[CH * NWORDS];
  __shared__ double s_wy[CH];
  __shared__ double s_x[NP], s_phi[NP], s_red[NT / 64];
  __shared__ int s_cnt[NP];
  __shared__ double s_lambda;
  const int tid = threadIdx.x, P = a.num_players, M = a.num_samples;
  const int BT = a.batch * a.num_targets;
  const double* L = a.factor;
  const double* tail = a.factor + (size_t)P * P;           // u (P), 1^T u, the smallest pivot, ok, the sum of the weights
  const bool ok = tail[P + 2] == 1.0;
  const int wt = (tid >> 5) < NWORDS ? (tid >> 5) : 0;
  const unsigned bt = 1u << (tid & 31);
  for (int item = blockIdx.x; item < BT; item += gridDim.x) {
    const double v0 = (double)a.v_empty[item], delta = (double)a.v_full[item] - v0;
    double acc = 0.0;
    for (int m0 = 0; m0 < M; m0 += CH) {
      const int n = min(CH, M - m0);
      __syncthreads();
      for (int q = tid; q < n * NWORDS; q += NT) s_bits[q] = a.bits[(size_t)m0 * NWORDS + q];
      for (int q = tid; q < n; q += NT)
        s_wy[q] = __dmul_rn(a.weights[m0 + q], (double)a.values[(size_t)(m0 + q) * BT + item] - v0);
      __syncthreads();
      if (tid < P)
        for (int m = 0; m < n; ++m)
          if (s_bits[m * NWORDS + wt] & bt) acc = __dadd_rn(acc, s_wy[m]);
    }
    if (tid < NP) {
      s_x[tid] = tid < P ? acc : 0.0;
      s_cnt[tid] = 0;
    }
    __syncthreads();
    if (ok) {
      for (int k = 0; k < P; ++k) {                       // L y = b
        if (tid == 0) s_x[k] /= L[(size_t)k * P + k];
        __syncthreads();
        const double yk = s_x[k];
        for (int r = k + 1 + tid; r < P; r += NT) s_x[r] -= L[(size_t)r * P + k] * yk;
        __syncthreads();
      }
      for (int k = P - 1; k >= 0; --k) {                  // L^T x = y
        if (tid == 0) s_x[k] /= L[(size_t)k * P + k];
        __syncthreads();
        const double xk = s_x[k];
        for (int r = tid; r < k; r += NT) s_x[r] -= L[(size_t)k * P + r] * xk;
        __syncthreads();
      }
      if (tid == 0) {
        double sx = 0.0;
        for (int i = 0; i < P; ++i) sx += s_x[i];
        s_lambda = (sx - delta) / tail[P];
      }
      __syncthreads();
    }
    if (tid < P) {
      const double phi = ok ? s_x[tid] - s_lambda * tail[tid] : __builtin_nan("");
      s_phi[tid] = phi;
      a.phi[(size_t)item * P + tid] = phi;
      a.phi32[(size_t)item * P + tid] = (float)phi;
    }
    int pl = 0;
    if (a.players && tid < NP) {
      pl = a.players[tid];
      pl = pl < 0 ? 0 : (pl > P - 1 ? P - 1 : pl);
      atomicAdd(&s_cnt[pl], 1);                           // integer, LDS
    }
    __syncthreads();
    if (a.players && a.patch_map && tid < NP) a.patch_map[(size_t)item * NP + tid] = (float)(s_phi[pl] / (double)s_cnt[pl]);
    double part = 0.0;                                    // sum_m w_m (z_m . phi - y_m)^2: a thread's samples in m order, then the fixed tree
    for (int m = tid; m < M; m += NT) {
      double pred = 0.0;
      for (int w = 0; w < NWORDS; ++w) {
        unsigned word = a.bits[(size_t)m * NWORDS + w];
        while (word) {
          const int i = 32 * w + __ffs(word) - 1;
          word &= word - 1u;
          if (i < P) pred += s_phi[i];
        }
      }
      const double r = pred - ((double)a.values[(size_t)m * BT + item] - v0);
      part += a.weights[m] * r * r;
    }
    const double tot = block_sum_t<NT / 64>(part, s_red);
    if (tid == 0) {
      a.fit_rmse[item] = sqrt(tot / tail[P + 3]);
      a.ok[item] = ok ? 1 : 0;
    }
  }
}

}  // namespace

extern "C" int rovit_shap_coalitions(const rovit_shap_coalition_args* p, rovit_stream_t stream) {
  const char* who = "shap_coalitions";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(sizes_ok(p->num_players, p->num_samples) && p->num_samples % 2 == 0, ROVIT_ERR_SHAPE,
                  "%s: %d players, %d samples (players 2..%d; samples even, 2..%d)", who, p->num_players, p->num_samples, NP, ROVIT_SHAP_MAX_SAMPLES);
  ROVIT_CHECK_ARG(p->pairs && p->pair_weights && p->bits && p->weights, ROVIT_ERR_NULL, "%s: a plan table, the bits or the weights are missing (null pointer)", who);
  ROVIT_CHECK_ARG((!p->src_replace && !p->src_drop) || p->players, ROVIT_ERR_NULL, "%s: src rows need the patch -> player map (null pointer)", who);
  ROVIT_CHECK_ARG(!p->src_drop || (p->drop_offsets && p->drop_words >= 1), ROVIT_ERR_NULL, "%s: src_drop needs drop_offsets and drop_words >= 1", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->pairs, 4) && rovit_aligned(p->pair_weights, 8) && rovit_aligned(p->players, 4) && rovit_aligned(p->drop_offsets, 8) &&
                      rovit_aligned(p->bits, 4) && rovit_aligned(p->weights, 8) && rovit_aligned(p->src_replace, 4) && rovit_aligned(p->src_drop, 4),
                  ROVIT_ERR_ALIGN, "%s: a pointer is not aligned to its element size", who);
  hipLaunchKernelGGL(shap_coalitions_kernel, dim3(capped(p->num_samples / 2, p->max_workgroups)), dim3(NT), 0, (hipStream_t)stream, *p);
  ROVIT_CHECK_LAUNCH("shap_coalitions_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_shap_gram(const rovit_shap_gram_args* p, rovit_stream_t stream) {
  const char* who = "shap_gram";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(sizes_ok(p->num_players, p->num_samples), ROVIT_ERR_SHAPE, "%s: %d players, %d samples (players 2..%d; samples 1..%d)", who,
                  p->num_players, p->num_samples, NP, ROVIT_SHAP_MAX_SAMPLES);
  ROVIT_CHECK_ARG(p->bits && p->weights && p->gram && p->factor, ROVIT_ERR_NULL, "%s: the bits, the weights, the matrix or the factor block is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->bits, 4) && rovit_aligned(p->weights, 8) && rovit_aligned(p->gram, 8) && rovit_aligned(p->factor, 8), ROVIT_ERR_ALIGN,
                  "%s: a pointer is not aligned to its element size", who);
  const int P = p->num_players, items = (P * (P + 1) / 2 + NT - 1) / NT;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(shap_gram_kernel, dim3(capped(items, p->max_workgroups)), dim3(NT), 0, s, *p, items);
  ROVIT_CHECK_LAUNCH("shap_gram_kernel");
  hipLaunchKernelGGL(shap_chol_kernel, dim3(1), dim3(NT_CHOL), 0, s, p->factor, P, p->weights, p->num_samples);
  ROVIT_CHECK_LAUNCH("shap_chol_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_shap_solve(const rovit_shap_solve_args* p, rovit_stream_t stream) {
  const char* who = "shap_solve";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(sizes_ok(p->num_players, p->num_samples), ROVIT_ERR_SHAPE, "%s: %d players, %d samples (players 2..%d; samples 1..%d)", who,
                  p->num_players, p->num_samples, NP, ROVIT_SHAP_MAX_SAMPLES);
  ROVIT_CHECK_ARG(p->batch >= 1 && p->num_targets >= 1 && (long long)p->batch * p->num_targets <= (1 << 20), ROVIT_ERR_SHAPE,
                  "%s: %d images x %d targets (>= 1 each, at most 2^20 together)", who, p->batch, p->num_targets);
  ROVIT_CHECK_ARG(p->bits && p->weights && p->factor && p->values && p->v_empty && p->v_full, ROVIT_ERR_NULL,
                  "%s: the bits, the weights, the factor block or the values are missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->phi && p->phi32 && p->fit_rmse && p->ok, ROVIT_ERR_NULL, "%s: an output is missing (null pointer)", who);
  ROVIT_CHECK_ARG(!p->patch_map || p->players, ROVIT_ERR_NULL, "%s: the patch map needs the patch -> player map (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->bits, 4) && rovit_aligned(p->weights, 8) && rovit_aligned(p->factor, 8) && rovit_aligned(p->values, 4) &&
                      rovit_aligned(p->v_empty, 4) && rovit_aligned(p->v_full, 4) && rovit_aligned(p->players, 4) && rovit_aligned(p->phi, 8) &&
                      rovit_aligned(p->phi32, 4) && rovit_aligned(p->patch_map, 4) && rovit_aligned(p->fit_rmse, 8) && rovit_aligned(p->ok, 4),
                  ROVIT_ERR_ALIGN, "%s: a pointer is not aligned to its element size", who);
  hipLaunchKernelGGL(shap_solve_kernel, dim3(capped((long long)p->batch * p->num_targets, p->max_workgroups)), dim3(NT), 0, (hipStream_t)stream, *p);
  ROVIT_CHECK_LAUNCH("shap_solve_kernel");
  return ROVIT_OK;
}
