// Selective prediction on the device: risk-coverage curves, AURC and the accept thresholds of the accumulator's recorded rows
// (rovit_eval_selective).  It is the first reader of the `uncertainty` column that rovit_eval_accumulate records.
//
// Reference being extended: evaluation/evaluator.py:35,64-65 collects all_uncertainties and never scores them.
//
// Seven kernels on the caller's stream behind two memset nodes (the counts with the permutations, and the WHOLE result block):
//   sel_prepare_kernel   one thread per row: the S score keys and the K risks in fp32 (columns of one (S + K, n) matrix), the four
//                        integer counters through LDS and integer atomics.
//   sel_rank_kernel      every column ONCE: each thread owns one x_i, tiles of x_j are staged in LDS and read as broadcasts;
//                        less = #{x_j < x_i}, eq = #{x_j == x_i}, before = #{j < i : x_j == x_i} are uint32 counts added with integer
//                        atomics, because the j range is split over workgroups.  Only the tiles that straddle the block's own rows
//                        compare indices; the tiles before them add their whole eq count, the tiles after them nothing.
//   sel_perm_kernel      perm[less + before] = row: the stable sort of each column, a bijection when every key is a number.
//   sel_scan_kernel      per (pair, 256-slot chunk): the risks gathered in sorted order, widened, and their inclusive prefix sums
//                        inside the chunk (Kogge-Stone over 256 slots: a fixed tree); the chunk total.
//   sel_offsets_kernel   per pair: the exclusive prefix sums of the chunk totals (16 totals per thread in order, then Kogge-Stone).
//   sel_risk_kernel      per (pair, chunk): r_k of every slot from the prefix sums and the tie-group bounds, and the chunk's sum of
//                        r_k in a fixed tree.
//   sel_final_kernel     per pair: the chunk sums in a fixed order, the P curve points (recomputed by the same device function, hence
//                        the same bits), mean = r_n and the thresholds.
// A pair is (score s, risk k), q = s K + k, or (risk k, risk k), q = S K + k: the oracle.  Work items are walked with a stride of the
// grid, and no item's result depends on which workgroup computes it: the grid cap changes nothing.  No floating-point atomics.
// rovit_eval_selective_ex with ROVIT_RANK_SORT replaces sel_rank_kernel and sel_perm_kernel only: the S + K columns are sorted in one
// batched call (sort_rank.hip), whose perm IS the stable order, and less, eq and before follow from two searches per sorted slot.
#include "common.h"
#include "rank_count.h"
#include "sort_device.h"

namespace {

constexpr int NT = 256;                 // threads per workgroup = slots per chunk
constexpr int MS = ROVIT_EVAL_SEL_MAX_SCORES, MK = ROVIT_EVAL_SEL_MAX_RISKS, MP = ROVIT_EVAL_SEL_MAX_COVERAGES;
static_assert(NT == 256, "prefix_at shifts a slot by 8 to find its chunk");
static_assert(NT == RANK_NT, "rank_stage_tile strides by RANK_NT");
constexpr int OFFS_PER_THREAD = (ROVIT_EVAL_MAX_ROWS / NT + NT - 1) / NT;          // 16 chunk totals per thread at the row limit

struct Layout {                          // byte offsets inside the workspace; every section starts on 16 bytes
  size_t x, cnt, perm, local, csum, rsum, total;
};
inline Layout layout(int n, int S, int K) {
  const size_t cols = (size_t)S + K, Q = (size_t)S * K + K, chunks = ((size_t)n + NT - 1) / NT;
  Layout l;
  l.x = 0;
  l.cnt = l.x + rovit_up16(cols * n * 4);
  l.perm = l.cnt + rovit_up16(3 * cols * n * 4);    // cnt and perm are contiguous: one memset covers both
  l.local = l.perm + rovit_up16(cols * n * 4);
  l.csum = l.local + rovit_up16(Q * n * 8);
  l.rsum = l.csum + rovit_up16(Q * chunks * 8);
  l.total = l.rsum + rovit_up16(Q * chunks * 8);
  return l;
}

struct Args {                            // what every kernel after the prepare needs
  int n, S, K, P, chunks;
  const float* x;                        // (S + K, n): scores, then risks
  unsigned* cnt;                         // (S + K, 3, n): less, eq, before
  unsigned* perm;                        // (S + K, n)
  double* local;                         // (Q, n)
  double* csum;                          // (Q, chunks): chunk totals, then their exclusive prefix sums
  double* rsum;                          // (Q, chunks)
  void* result;
};

__device__ __forceinline__ int pair_column(const Args& a, int q) { return q < a.S * a.K ? q / a.K : a.S + (q - a.S * a.K); }
__device__ __forceinline__ int pair_risk(const Args& a, int q) { return q < a.S * a.K ? q % a.K : q - a.S * a.K; }

// inclusive prefix sums of one value per thread over the workgroup: Kogge-Stone in LDS, the same tree for every launch
__device__ __forceinline__ double block_scan(double v, double* s) {
  const int tid = threadIdx.x;
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    const double t = tid >= d ? s[tid - d] : 0.0;
    __syncthreads();
    if (tid >= d) s[tid] += t;
    __syncthreads();
  }
  return s[tid];
}

__global__ __launch_bounds__(NT) void sel_prepare_kernel(const rovit_eval_sel a, float* __restrict__ x, int chunks) {
  __shared__ unsigned s_cnt[4];
  const int tid = threadIdx.x, n = a.n, C = a.num_classes, S = a.num_scores, K = a.num_risks;
  for (int w = blockIdx.x; w < chunks; w += gridDim.x) {
    __syncthreads();
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();
    const int i = w * NT + tid;
    if (i < n) {
      float pmax = 0.f, plogp = 0.f;
      bool pnan = false;
      for (int c = 0; c < C; ++c) {
        const float p = a.probs[(size_t)i * C + c];
        pnan |= p != p;
        pmax = c == 0 || p > pmax ? p : pmax;
        plogp += p == 0.f ? 0.f : p * logf(p);
      }
      if (pnan) pmax = __builtin_nanf("");                    // np.max propagates a NaN
      const int lab = a.label[i];
      unsigned bad_key = 0, bad_risk = 0, neg_risk = 0;
      for (int s = 0; s < S; ++s) {
        float v;
        switch (a.score_kind[s]) {
          case ROVIT_EVAL_SEL_CONFIDENCE: v = 1.0f - pmax; break;
          case ROVIT_EVAL_SEL_ENTROPY: v = 0.f - plogp; break;                // +0 for a certain row
          case ROVIT_EVAL_SEL_SIGMA: v = a.uncertainty[i]; break;
          default: v = a.score_column[s][i]; break;
        }
        bad_key += !isfinite(v);
        x[(size_t)s * n + i] = v;
        if (a.keys_out) a.keys_out[(size_t)s * n + i] = v;
      }
      for (int k = 0; k < K; ++k) {
        float v;
        switch (a.risk_kind[k]) {
          case ROVIT_EVAL_SEL_ERROR: v = a.pred[i] != lab ? 1.0f : 0.0f; break;
          case ROVIT_EVAL_SEL_ABS_ERR: v = fabsf(a.sev_true[i] - a.sev_pred[i]); break;
          default: v = a.risk_column[k][i]; break;
        }
        bad_risk += !isfinite(v);
        neg_risk += v < 0.f;
        x[(size_t)(S + k) * n + i] = v;
        if (a.risks_out) a.risks_out[(size_t)k * n + i] = v;
      }
      if (bad_key) atomicAdd(&s_cnt[0], bad_key);
      if (bad_risk) atomicAdd(&s_cnt[1], bad_risk);
      if (neg_risk) atomicAdd(&s_cnt[2], neg_risk);
      if (lab < 0) atomicAdd(&s_cnt[3], 1u);
    }
    __syncthreads();
    if (tid < 4 && s_cnt[tid]) atomicAdd(&((unsigned long long*)a.result)[ROVIT_EVAL_SEL_NONFINITE_KEYS + tid], (unsigned long long)s_cnt[tid]);
  }
  if (blockIdx.x == 0 && tid == 0) ((long long*)a.result)[ROVIT_EVAL_SEL_N] = n;
}

__global__ __launch_bounds__(NT) void sel_rank_kernel(const Args a, int splits, int tiles_per_split) {
  __shared__ __attribute__((aligned(16))) float sX[RANK_RT];
  const int n = a.n, tid = threadIdx.x, cols = a.S + a.K;
  const int ntiles = (n + RANK_RT - 1) / RANK_RT;
  const int items = a.chunks * splits * cols;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int chunk = w % a.chunks, split = (w / a.chunks) % splits, col = w / (a.chunks * splits);
    const float* X = a.x + (size_t)col * n;
    const int i0 = chunk * NT, i = i0 + tid;
    const float xi = i < n ? X[i] : 0.f;
    unsigned less = 0, eq = 0, before = 0;
    const int t0 = split * tiles_per_split, t1 = min(ntiles, t0 + tiles_per_split);
    for (int t = t0; t < t1; ++t) {
      __syncthreads();
      const int j0 = t * RANK_RT;
      rank_stage_tile(sX, X, j0, n);
      __syncthreads();
      unsigned e = 0;
      if (j0 + RANK_RT <= i0 || j0 >= i0 + NT) {          // every j of the tile lies before, or after, every row of the block
        rank_count_tile(sX, xi, less, e);
        if (j0 + RANK_RT <= i0) before += e;
      } else {
        rank_count_tile<true>(sX, xi, less, e, &before, i - j0);          // j < i  <=>  k < i - j0
      }
      eq += e;
    }
    if (i < n) {
      unsigned* c = a.cnt + (size_t)col * 3 * n;
      atomicAdd(&c[i], less);
      atomicAdd(&c[(size_t)n + i], eq);
      atomicAdd(&c[2 * (size_t)n + i], before);
    }
  }
}

__global__ __launch_bounds__(NT) void sel_perm_kernel(const Args a) {
  const int n = a.n, items = a.chunks * (a.S + a.K);
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int chunk = w % a.chunks, col = w / a.chunks;
    const int i = chunk * NT + threadIdx.x;
    if (i < n) {
      const unsigned* c = a.cnt + (size_t)col * 3 * n;
      const unsigned slot = c[i] + c[2 * (size_t)n + i];
      if (slot < (unsigned)n) a.perm[(size_t)col * n + slot] = (unsigned)i;          // always, when the keys are numbers
    }
  }
}

__global__ __launch_bounds__(NT) void sel_scan_kernel(const Args a) {
  __shared__ double s_scan[NT];
  const int n = a.n, tid = threadIdx.x, Q = a.S * a.K + a.K;
  const int items = a.chunks * Q;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int chunk = w % a.chunks, q = w / a.chunks;
    const int col = pair_column(a, q), k = pair_risk(a, q);
    const int j = chunk * NT + tid;
    double v = 0.0;
    if (j < n) {
      const unsigned row = min(a.perm[(size_t)col * n + j], (unsigned)(n - 1));
      v = (double)a.x[(size_t)(a.S + k) * n + row];
    }
    const double incl = block_scan(v, s_scan);
    if (j < n) a.local[(size_t)q * n + j] = incl;
    if (tid == NT - 1) a.csum[(size_t)q * a.chunks + chunk] = incl;
  }
}

__global__ __launch_bounds__(NT) void sel_offsets_kernel(const Args a) {
  __shared__ double s_scan[NT];
  const int tid = threadIdx.x, Q = a.S * a.K + a.K, chunks = a.chunks;
  for (int q = blockIdx.x; q < Q; q += gridDim.x) {
    double* cs = a.csum + (size_t)q * chunks;
    double v[OFFS_PER_THREAD];
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < OFFS_PER_THREAD; ++r) {
      const int c = tid * OFFS_PER_THREAD + r;
      v[r] = c < chunks ? cs[c] : 0.0;
      t += v[r];
    }
    block_scan(t, s_scan);
    double run = tid == 0 ? 0.0 : s_scan[tid - 1];          // exclusive over the threads
#pragma unroll
    for (int r = 0; r < OFFS_PER_THREAD; ++r) {
      const int c = tid * OFFS_PER_THREAD + r;
      if (c < chunks) cs[c] = run;
      run += v[r];
    }
  }
}

// Pref[j]: the sum of the first j sorted risks of pair q
__device__ __forceinline__ double prefix_at(const Args& a, int q, int j) {
  return j <= 0 ? 0.0 : a.csum[(size_t)q * a.chunks + ((j - 1) >> 8)] + a.local[(size_t)q * a.n + (j - 1)];
}
// r_k, 1 <= k <= n: the row in sorted slot k - 1 knows its tie group [g, g + m)
__device__ __forceinline__ double selective_risk(const Args& a, int q, int col, int k) {
  const int n = a.n;
  const unsigned row = min(a.perm[(size_t)col * n + (k - 1)], (unsigned)(n - 1));
  const unsigned* c = a.cnt + (size_t)col * 3 * n;
  const int g = min((int)c[row], k - 1);
  const int m = max(1, min((int)c[(size_t)n + row], n - g));
  const double pg = prefix_at(a, q, g), pgm = prefix_at(a, q, g + m);
  return (pg + (double)(k - g) * (pgm - pg) / (double)m) / (double)k;
}

__global__ __launch_bounds__(NT) void sel_risk_kernel(const Args a) {
  __shared__ double s_d[4];
  const int n = a.n, tid = threadIdx.x, Q = a.S * a.K + a.K;
  const int items = a.chunks * Q;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int chunk = w % a.chunks, q = w / a.chunks;
    const int k = chunk * NT + tid + 1;
    const double r = k <= n ? selective_risk(a, q, pair_column(a, q), k) : 0.0;
    const double s = block_sum_t(r, s_d);
    if (tid == 0) a.rsum[(size_t)q * a.chunks + chunk] = s;
  }
}

__global__ __launch_bounds__(NT) void sel_final_kernel(const Args a) {
  __shared__ double s_d[4];
  const int n = a.n, tid = threadIdx.x, S = a.S, K = a.K, P = a.P, Q = S * K + K;
  double* res = (double*)a.result;
  const size_t risk_base = ROVIT_EVAL_SEL_HEADER, pair_base = risk_base + (size_t)K * (2 + P), thr_base = pair_base + (size_t)S * K * (1 + P);
  for (int q = blockIdx.x; q < Q; q += gridDim.x) {
    const int col = pair_column(a, q), kr = pair_risk(a, q);
    const bool oracle = q >= S * K;
    double s = 0.0;
    for (int c = tid; c < a.chunks; c += NT) s += a.rsum[(size_t)q * a.chunks + c];
    s = block_sum_t(s, s_d) / (double)n;
    double* out = oracle ? res + risk_base + (size_t)kr * (2 + P) + 1 : res + pair_base + (size_t)q * (1 + P);
    if (tid == 0) {
      out[0] = s;
      if (oracle) out[-1] = selective_risk(a, q, col, n);     // mean = r_n
    }
    for (int p = tid + 1; p <= P; p += NT) {
      const int kp = (int)(((long long)p * n + P - 1) / P);
      out[p] = selective_risk(a, q, col, kp);
      if (!oracle && kr == 0) {
        const unsigned row = min(a.perm[(size_t)col * n + (kp - 1)], (unsigned)(n - 1));
        res[thr_base + (size_t)col * P + (p - 1)] = (double)a.x[(size_t)col * n + row];
      }
    }
  }
}

static inline bool limits_ok(int n, int S, int K) {
  return n >= 1 && n <= ROVIT_EVAL_MAX_ROWS && S >= 1 && S <= MS && K >= 1 && K <= MK;
}

}  // namespace

extern "C" size_t rovit_eval_selective_workspace_bytes(int n, int S, int K) { return limits_ok(n, S, K) ? layout(n, S, K).total : 0; }

namespace {
// the rank workspace of the sorted score card: the sorted keys of the S + K columns, then the sort's own
struct SelRankLayout { size_t keys, sort, total; };
inline SelRankLayout sel_rank_layout(int n, int cols) {
  int nn[ROVIT_SORT_MAX_COLUMNS];
  for (int c = 0; c < cols; ++c) nn[c] = n;
  SelRankLayout l;
  l.keys = 0;
  l.sort = l.keys + (size_t)cols * rovit_up16((size_t)n * 4);
  l.total = l.sort + rovit_sort_batch_workspace_bytes(nn, cols);
  return l;
}
static_assert(MS + MK <= ROVIT_SORT_MAX_COLUMNS, "every column of a score card fits one batched sort");
}  // namespace

extern "C" size_t rovit_eval_selective_rank_workspace_bytes(int n, int S, int K) {
  return limits_ok(n, S, K) ? sel_rank_layout(n, S + K).total : 0;
}

extern "C" int rovit_eval_selective(const rovit_eval_sel* p, rovit_stream_t stream) {
  return rovit_eval_selective_ex(p, ROVIT_RANK_COUNT, nullptr, 0, stream);
}

extern "C" int rovit_eval_selective_ex(const rovit_eval_sel* p, int method, void* rank_workspace, size_t rank_workspace_bytes,
                                       rovit_stream_t stream) {
  const char* who = "eval_selective";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_EVAL_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d recorded rows (1..%d)", who, p->n, ROVIT_EVAL_MAX_ROWS);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= ROVIT_EVAL_MAX_CLASSES, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who,
                  p->num_classes, ROVIT_EVAL_MAX_CLASSES);
  ROVIT_CHECK_ARG(p->num_scores >= 1 && p->num_scores <= MS, ROVIT_ERR_SHAPE, "%s: %d scores (1..%d)", who, p->num_scores, MS);
  ROVIT_CHECK_ARG(p->num_risks >= 1 && p->num_risks <= MK, ROVIT_ERR_SHAPE, "%s: %d risks (1..%d)", who, p->num_risks, MK);
  ROVIT_CHECK_ARG(p->num_coverages >= 1 && p->num_coverages <= MP, ROVIT_ERR_SHAPE, "%s: %d coverages (1..%d)", who, p->num_coverages, MP);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  const int n = p->n, S = p->num_scores, K = p->num_risks, P = p->num_coverages;
  bool need_sigma = false, need_class = false, need_sev = false;
  for (int s = 0; s < S; ++s) {
    const int kind = p->score_kind[s];
    ROVIT_CHECK_ARG(kind >= ROVIT_EVAL_SEL_CONFIDENCE && kind <= ROVIT_EVAL_SEL_SCORE_COLUMN, ROVIT_ERR_SHAPE, "%s: score %d has the unknown kind %d",
                    who, s, kind);
    ROVIT_CHECK_ARG(kind != ROVIT_EVAL_SEL_SCORE_COLUMN || p->score_column[s], ROVIT_ERR_NULL, "%s: score %d is a column with a null pointer", who, s);
    ROVIT_CHECK_ARG(kind != ROVIT_EVAL_SEL_SCORE_COLUMN || rovit_aligned(p->score_column[s], 4), ROVIT_ERR_ALIGN,
                    "%s: the column of score %d is not aligned to its element size", who, s);
    need_sigma |= kind == ROVIT_EVAL_SEL_SIGMA;
  }
  for (int k = 0; k < K; ++k) {
    const int kind = p->risk_kind[k];
    ROVIT_CHECK_ARG(kind >= ROVIT_EVAL_SEL_ERROR && kind <= ROVIT_EVAL_SEL_RISK_COLUMN, ROVIT_ERR_SHAPE, "%s: risk %d has the unknown kind %d", who,
                    k, kind);
    ROVIT_CHECK_ARG(kind != ROVIT_EVAL_SEL_RISK_COLUMN || p->risk_column[k], ROVIT_ERR_NULL, "%s: risk %d is a column with a null pointer", who, k);
    ROVIT_CHECK_ARG(kind != ROVIT_EVAL_SEL_RISK_COLUMN || rovit_aligned(p->risk_column[k], 4), ROVIT_ERR_ALIGN,
                    "%s: the column of risk %d is not aligned to its element size", who, k);
    need_class |= kind == ROVIT_EVAL_SEL_ERROR;
    need_sev |= kind == ROVIT_EVAL_SEL_ABS_ERR;
  }
  // the prepare reads probs and label of every row whatever the kinds are (the label counter): both are always required
  ROVIT_CHECK_ARG(p->probs && p->label && (!need_class || p->pred) && (!need_sev || (p->sev_pred && p->sev_true)) && (!need_sigma || p->uncertainty),
                  ROVIT_ERR_NULL, "%s: a record array is missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->workspace && p->result, ROVIT_ERR_NULL, "%s: the workspace or the result block is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->probs) && rovit_aligned16(p->pred) && rovit_aligned16(p->label) && rovit_aligned16(p->sev_pred) &&
                      rovit_aligned16(p->sev_true) && rovit_aligned16(p->uncertainty),
                  ROVIT_ERR_ALIGN, "%s: a record array is not 16-byte aligned", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->workspace) && rovit_aligned(p->result, 8) && rovit_aligned(p->keys_out, 4) && rovit_aligned(p->risks_out, 4),
                  ROVIT_ERR_ALIGN, "%s: the workspace, the result block or a matrix to leave behind is not aligned", who);
  const Layout l = layout(n, S, K);
  ROVIT_CHECK_ARG(p->workspace_bytes >= l.total, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes,
                  l.total);

  ROVIT_CHECK_ARG(method >= ROVIT_RANK_AUTO && method <= ROVIT_RANK_SORT, ROVIT_ERR_SHAPE, "%s: unknown rank method %d", who, method);
  const bool sorted = rovit_rank_method(method, n) == ROVIT_RANK_SORT;
  const SelRankLayout rl = sel_rank_layout(n, S + K);
  if (sorted) {
    ROVIT_CHECK_ARG(rank_workspace, ROVIT_ERR_NULL, "%s: the rank workspace is missing (null pointer)", who);
    ROVIT_CHECK_ARG(rovit_aligned16(rank_workspace), ROVIT_ERR_ALIGN, "%s: the rank workspace is not 16-byte aligned", who);
    ROVIT_CHECK_ARG(rank_workspace_bytes >= rl.total, ROVIT_ERR_SHAPE, "%s: the rank workspace holds %zu bytes, %zu are needed", who,
                    rank_workspace_bytes, rl.total);
  }
  char* ws = (char*)p->workspace;
  Args a;
  a.n = n; a.S = S; a.K = K; a.P = P; a.chunks = (n + NT - 1) / NT;
  a.x = (const float*)(ws + l.x);
  a.cnt = (unsigned*)(ws + l.cnt);
  a.perm = (unsigned*)(ws + l.perm);
  a.local = (double*)(ws + l.local);
  a.csum = (double*)(ws + l.csum);
  a.rsum = (double*)(ws + l.rsum);
  a.result = p->result;
  const int cols = S + K, Q = S * K + K, ntiles = (n + RANK_RT - 1) / RANK_RT;
  const size_t words = ROVIT_EVAL_SEL_WORDS(S, K, P);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(a.cnt, 0, l.local - l.cnt, s) != hipSuccess || hipMemsetAsync(p->result, 0, words * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  const long long cap = p->max_workgroups > 0 ? p->max_workgroups : (1ll << 30);
  auto grid = [&](long long items) { return dim3((unsigned)(items < cap ? items : cap)); };
  // split the j range until about 1024 workgroups exist; the counts are integers, so the split changes nothing
  int splits = (1024 + a.chunks * cols - 1) / (a.chunks * cols);
  splits = splits < 1 ? 1 : (splits > ntiles ? ntiles : splits);
  const int tps = (ntiles + splits - 1) / splits;
  splits = (ntiles + tps - 1) / tps;
  hipLaunchKernelGGL(sel_prepare_kernel, grid(a.chunks), dim3(NT), 0, s, *p, (float*)(ws + l.x), a.chunks);
  ROVIT_CHECK_LAUNCH("sel_prepare_kernel");
  if (sorted) {
    // the sort's perm IS the stable order; less, eq and before of the row in every sorted slot by two searches in the sorted keys
    char* rws = (char*)rank_workspace;
    RovitSortCol c[ROVIT_SORT_MAX_COLUMNS];
    RovitRankSlots r[ROVIT_SORT_MAX_COLUMNS];
    for (int k = 0; k < cols; ++k) {
      unsigned* keys = (unsigned*)(rws + rl.keys + (size_t)k * rovit_up16((size_t)n * 4));
      unsigned* perm = a.perm + (size_t)k * n;
      unsigned* cnt = a.cnt + (size_t)k * 3 * n;
      c[k] = RovitSortCol{a.x + (size_t)k * n, keys, perm, n};
      r[k] = RovitRankSlots{keys, perm, n, cnt, cnt + (size_t)n, cnt + 2 * (size_t)n};
    }
    int rc = rovit_sort_batch(c, cols, rws + rl.sort, rank_workspace_bytes - rl.sort, p->max_workgroups, s, who);
    if (rc != ROVIT_OK) return rc;
    rc = rovit_rank_slots(r, cols, p->max_workgroups, s, who);
    if (rc != ROVIT_OK) return rc;
  } else {
    hipLaunchKernelGGL(sel_rank_kernel, grid((long long)a.chunks * splits * cols), dim3(NT), 0, s, a, splits, tps);
    ROVIT_CHECK_LAUNCH("sel_rank_kernel");
    hipLaunchKernelGGL(sel_perm_kernel, grid((long long)a.chunks * cols), dim3(NT), 0, s, a);
    ROVIT_CHECK_LAUNCH("sel_perm_kernel");
  }
  hipLaunchKernelGGL(sel_scan_kernel, grid((long long)a.chunks * Q), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("sel_scan_kernel");
  hipLaunchKernelGGL(sel_offsets_kernel, grid(Q), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("sel_offsets_kernel");
  hipLaunchKernelGGL(sel_risk_kernel, grid((long long)a.chunks * Q), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("sel_risk_kernel");
  hipLaunchKernelGGL(sel_final_kernel, grid(Q), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("sel_final_kernel");
  return ROVIT_OK;
}
