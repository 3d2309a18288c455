// Split conformal prediction on the evaluation record: rovit_eval_conformal (the fit) and rovit_eval_conformal_apply (test rows and
// deployment).  Definitions and block layouts: include/rovit_hip.h.  The reference has nothing of the kind.
//
// The fit, on the caller's stream behind two memset nodes (counters, select state and histograms; the WHOLE result block):
//   conf_score_kernel   one thread per row: the M score columns (conformal_device.h), a 16-bit word per row with the validity bits and
//                       the true class, the per (column, class) row counts through LDS and integer atomics.
//   conf_init_kernel    one thread per entry (column, group, level): n_g, k in 64-bit integers, trivial entries finished here.
//   4 x conf_hist_kernel + conf_step_kernel: a radix select, most significant byte first.  The histogram kernel walks
//                       (row chunk, column) items and counts byte d of every valid row whose higher bytes equal the entry's prefix,
//                       in an LDS histogram [group][level][256] sized from the descriptor, then adds the non-zero bins to the global
//                       histogram.  The step kernel gives an entry one wave: 4 bins per lane, a wave scan, the bin where the running
//                       count reaches the remaining rank; it appends the digit, keeps the rank inside the bin and clears the bins.
// O(n) per column and round, ten launches whatever the data are.  Only integer atomics; work items are walked with a stride of the
// grid and no item's contribution depends on which workgroup counts it: the grid cap changes nothing.
#include "common.h"
#include "conformal_device.h"

namespace {

using namespace conformal;

constexpr int NT = 256;                 // threads per workgroup = rows per score / apply chunk
constexpr int HR = 8;                   // rows per thread of one histogram item
constexpr int MS = ROVIT_EVAL_CONF_MAX_SCORES, MA = ROVIT_EVAL_CONF_MAX_LEVELS;
constexpr int NCNT = MS * MAXC + 2;     // rows per (column, class) | bad labels | labelled rows
constexpr int EW = ROVIT_EVAL_CONF_ENTRY_WORDS;

struct Layout {                          // byte offsets inside the fit's workspace; every section starts on 16 bytes
  size_t x, flags, cnt, prefix, krem, trivial, hist, total;
};
inline Layout layout(int n, int M, int G, int A) {
  const size_t E = (size_t)M * G * A;
  Layout l;
  l.x = 0;
  l.flags = l.x + rovit_up16((size_t)M * n * 4);
  l.cnt = l.flags + rovit_up16((size_t)n * 2);
  l.prefix = l.cnt + rovit_up16(NCNT * 4);    // cnt .. hist are contiguous: one memset covers them
  l.krem = l.prefix + rovit_up16(E * 4);
  l.trivial = l.krem + rovit_up16(E * 4);
  l.hist = l.trivial + rovit_up16(E * 4);
  l.total = l.hist + rovit_up16(E * 256 * 4);
  return l;
}

struct Fit {                             // what the kernels after the scores need
  int n, M, G, A, E;
  const float* x;                        // (M, n)
  const unsigned short* flags;           // (n): bit m = row valid for column m; high byte = true class
  const unsigned* cnt;                   // NCNT
  unsigned* prefix;                      // (E): the digits found so far, right-aligned
  unsigned* krem;                        // (E): the rank that remains inside the prefix
  unsigned* trivial;                     // (E)
  unsigned* hist;                        // (E, 256)
  long long* result;
};

__global__ __launch_bounds__(NT) void conf_score_kernel(const rovit_eval_conf a, float* __restrict__ x, unsigned short* __restrict__ flags,
                                                        unsigned* __restrict__ cnt, int chunks) {
  __shared__ unsigned s_cnt[NCNT];
  const int tid = threadIdx.x, n = a.n, C = a.num_classes, M = a.num_scores;
  for (int w = blockIdx.x; w < chunks; w += gridDim.x) {
    __syncthreads();
    for (int t = tid; t < NCNT; t += NT) s_cnt[t] = 0;
    __syncthreads();
    const int i = w * NT + tid;
    if (i < n) {
      const int lab = a.label[i];
      const bool ok = lab >= 0 && lab < C;
      Sorted s;
      sort_row(a.probs + (size_t)i * C, C, s);
      const float u = a.randomized ? draw_u(a.seed, a.row_offset + (unsigned)i) : 0.f;
      if (a.u_out) a.u_out[i] = u;
      unsigned bits = 0;
      for (int m = 0; m < M; ++m) {
        const int kind = a.score_kind[m];
        bool sigma_ok = true;
        float v;
        if (is_class_kind(kind)) v = ok ? class_score(kind, s, lab, u, a.raps_lambda, a.raps_k) : __builtin_nanf("");
        else v = row_score(a, m, i, sigma_ok);
        x[(size_t)m * n + i] = v;
        if (a.scores_out) a.scores_out[(size_t)m * n + i] = v;
        if (ok && sigma_ok && isfinite(v)) {
          bits |= 1u << m;
          atomicAdd(&s_cnt[m * MAXC + lab], 1u);
        }
      }
      flags[i] = (unsigned short)(bits | ((ok ? (unsigned)lab : 0xFFu) << 8));
      atomicAdd(&s_cnt[MS * MAXC + (ok ? 1 : 0)], 1u);
    }
    __syncthreads();
    for (int t = tid; t < NCNT; t += NT)
      if (s_cnt[t]) atomicAdd(&cnt[t], s_cnt[t]);
  }
}

__global__ __launch_bounds__(NT) void conf_init_kernel(const rovit_eval_conf a, const Fit f) {
  const int C = a.num_classes;
  for (int e = blockIdx.x * NT + threadIdx.x; e < f.E; e += gridDim.x * NT) {
    const int lvl = e % f.A, g = (e / f.A) % f.G, m = e / (f.A * f.G);
    long long ng = 0;
    for (int c = 0; c < C; ++c)
      if (g == 0 || g == 1 + c) ng += f.cnt[m * MAXC + c];
    const long long k = ng + 1 - ((ng + 1) * (long long)a.alpha_num[lvl]) / (long long)a.alpha_den[lvl];
    const bool trivial = k > ng;
    long long* out = f.result + ROVIT_EVAL_CONF_ENTRIES + (size_t)EW * e;
    out[0] = ng;
    out[1] = k;
    if (trivial) {
      out[2] = ng;
      out[3] = 0;
      out[4] = 0x7F800000ll;               // +inf
      out[5] = 1;
    }
    f.trivial[e] = trivial ? 1u : 0u;
    f.krem[e] = trivial ? 0u : (unsigned)k;
  }
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    const long long labelled = f.cnt[MS * MAXC + 1];
    if (t == 0) {
      f.result[ROVIT_EVAL_CONF_N] = a.n;
      f.result[ROVIT_EVAL_CONF_BAD_LABELS] = f.cnt[MS * MAXC];
      f.result[ROVIT_EVAL_CONF_N_LABELLED] = labelled;
    }
    if (t < f.M) {
      long long valid = 0;
      for (int c = 0; c < C; ++c) valid += f.cnt[t * MAXC + c];
      f.result[ROVIT_EVAL_CONF_BAD_ROWS + t] = labelled - valid;
    }
  }
}

// round r looks at byte 3 - r; dynamic LDS: prefix[GA] | histogram [GA][256]
__global__ __launch_bounds__(NT) void conf_hist_kernel(const Fit f, int round, int chunks) {
  extern __shared__ unsigned s_dyn[];
  const int tid = threadIdx.x, n = f.n, A = f.A, GA = f.G * f.A;
  unsigned* s_pre = s_dyn;
  unsigned* s_h = s_dyn + GA;
  const int shift = 24 - 8 * round;
  const int items = chunks * f.M;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int chunk = w % chunks, m = w / chunks;
    __syncthreads();
    for (int t = tid; t < GA; t += NT) s_pre[t] = f.prefix[m * GA + t];
    for (int t = tid; t < GA * 256; t += NT) s_h[t] = 0;
    __syncthreads();
    const float* X = f.x + (size_t)m * n;
#pragma unroll
    for (int r = 0; r < HR; ++r) {
      const int i = (chunk * HR + r) * NT + tid;
      if (i >= n) continue;
      const unsigned fl = f.flags[i];
      if (!((fl >> m) & 1u)) continue;
      const unsigned key = order_key(X[i]);
      const unsigned hi = round == 0 ? 0u : key >> (shift + 8), digit = (key >> shift) & 255u;
      for (int lvl = 0; lvl < A; ++lvl)
        if (hi == s_pre[lvl]) atomicAdd(&s_h[lvl * 256 + digit], 1u);
      if (f.G > 1) {
        const int g = 1 + (int)(fl >> 8);                       // a valid row's class is in [0, C) and G = 1 + C
        for (int lvl = 0; lvl < A; ++lvl)
          if (hi == s_pre[g * A + lvl]) atomicAdd(&s_h[(g * A + lvl) * 256 + digit], 1u);
      }
    }
    __syncthreads();
    unsigned* H = f.hist + (size_t)m * GA * 256;
    for (int t = tid; t < GA * 256; t += NT)
      if (s_h[t]) atomicAdd(&H[t], s_h[t]);
  }
}

// one wave per entry: lane l owns bins 4 l .. 4 l + 3
__global__ __launch_bounds__(64) void conf_step_kernel(const Fit f, int round) {
  const int lane = threadIdx.x;
  for (int e = blockIdx.x; e < f.E; e += gridDim.x) {
    uint4* H = reinterpret_cast<uint4*>(f.hist + (size_t)e * 256) + lane;
    const uint4 h = *H;
    *H = make_uint4(0u, 0u, 0u, 0u);                            // the next round counts into a clean histogram
    if (f.trivial[e]) continue;
    const unsigned kr = f.krem[e];
    const unsigned own = h.x + h.y + h.z + h.w;
    unsigned incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    const unsigned excl = incl - own;
    if (excl < kr && kr <= incl) {                              // exactly one lane: the running count reaches kr in its bins
      const unsigned v[4] = {h.x, h.y, h.z, h.w};
      unsigned below = excl, eq = 0;
      int bin = 4 * lane + 3;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (eq == 0) {
          if (kr <= below + v[j]) {
            bin = 4 * lane + j;
            eq = v[j];
          } else {
            below += v[j];
          }
        }
      }
      const unsigned prefix = round == 0 ? (unsigned)bin : (f.prefix[e] << 8) | (unsigned)bin;
      f.prefix[e] = prefix;
      f.krem[e] = kr - below;
      if (round == 3) {
        long long* out = f.result + ROVIT_EVAL_CONF_ENTRIES + (size_t)EW * e;
        out[2] = out[1] - (long long)(kr - below);              // rows below the threshold: k minus the rank inside its tie group
        out[3] = eq;
        out[4] = (long long)key_bits(prefix);
        out[5] = 0;
      }
    }
  }
}

// ---- the application ---------------------------------------------------------------------------------------------------------

// dynamic LDS: the tallies of one chunk, M (16 + 32 A) counters
__global__ __launch_bounds__(NT) void conf_apply_kernel(const rovit_eval_conf a, double* __restrict__ partials, int chunks, int G, int Mcls) {
  extern __shared__ unsigned s_dyn[];
  __shared__ double s_d[4];
  __shared__ unsigned s_bad[2];
  const int tid = threadIdx.x, n = a.n, C = a.num_classes, M = a.num_scores, A = a.num_levels;
  const int per = 16 + 32 * A, words = M * per;
  const bool tally = a.label != nullptr;
  unsigned long long* res = (unsigned long long*)a.result;
  for (int w = blockIdx.x; w < chunks; w += gridDim.x) {
    __syncthreads();
    if (tally) {
      for (int t = tid; t < words; t += NT) s_dyn[t] = 0;
      if (tid < 2) s_bad[tid] = 0;
    }
    __syncthreads();
    const int i = w * NT + tid;
    const bool live = i < n;
    int lab = -1;
    bool ok = false;
    Sorted s;
    float u = 0.f;
    if (live) {
      if (tally) {
        lab = a.label[i];
        ok = lab >= 0 && lab < C;
        atomicAdd(&s_bad[ok ? 1 : 0], 1u);
      }
      sort_row(a.probs + (size_t)i * C, C, s);
      if (a.randomized) u = draw_u(a.seed, a.row_offset + (unsigned)i);
    }
    int mc = 0;
    for (int m = 0; m < M; ++m) {
      const int kind = a.score_kind[m];
      unsigned* T = s_dyn + m * per;
      if (is_class_kind(kind)) {
        if (live) {
          float sc[MAXC];
#pragma unroll
          for (int c = 0; c < MAXC; ++c) sc[c] = c < C ? class_score(kind, s, c, u, a.raps_lambda, a.raps_k) : __builtin_nanf("");
          float sy = __builtin_nanf("");
#pragma unroll
          for (int c = 0; c < MAXC; ++c)
            if (c == lab) sy = sc[c];
          const bool valid = ok && isfinite(sy);
          if (valid) {
            atomicAdd(&T[0], 1u);
            atomicAdd(&T[8 + lab], 1u);
          } else if (ok) {
            atomicAdd(&T[1], 1u);
          }
          for (int lvl = 0; lvl < A; ++lvl) {
            unsigned mask = 0;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
              if (c < C) {
                const float q = a.thresholds[((size_t)m * G + (G > 1 ? 1 + c : 0)) * A + lvl];
                mask |= (sc[c] <= q ? 1u : 0u) << c;
              }
            }
            if (a.member_out) a.member_out[((size_t)i * Mcls + mc) * A + lvl] = (unsigned char)mask;
            if (valid) {
              unsigned* L = T + 16 + 32 * lvl;
              const int size = __popc(mask);
              atomicAdd(&L[size], 1u);
              if ((mask >> lab) & 1u) {
                atomicAdd(&L[9 + size], 1u);
                atomicAdd(&L[18 + lab], 1u);
                atomicAdd(&L[26], 1u);
              }
            }
          }
        }
        ++mc;
      } else if (tally) {
        double sg = 0.0;
        if (live) {
          bool sigma_ok = true;
          const float v = row_score(a, m, i, sigma_ok);
          const bool valid = ok && sigma_ok && isfinite(v);
          if (valid) {
            atomicAdd(&T[0], 1u);
            for (int lvl = 0; lvl < A; ++lvl)
              if (v <= a.thresholds[((size_t)m * G) * A + lvl]) atomicAdd(&T[16 + 32 * lvl + 26], 1u);
            if (kind == ROVIT_EVAL_CONF_MU_SCALED) sg = (double)a.uncertainty[i];
          } else if (ok) {
            atomicAdd(&T[1], 1u);
          }
        }
        if (kind == ROVIT_EVAL_CONF_MU_SCALED) {                 // uniform over the workgroup: every thread reaches the barriers
          const double t = block_sum_t(sg, s_d);
          if (tid == 0) partials[(size_t)m * chunks + w] = t;
        }
      }
    }
    if (tally) {
      __syncthreads();
      for (int t = tid; t < words; t += NT)
        if (s_dyn[t]) atomicAdd(&res[ROVIT_EVAL_CONF_APPLY_SCORES + t], (unsigned long long)s_dyn[t]);
      if (tid < 2 && s_bad[tid]) atomicAdd(&res[tid == 0 ? ROVIT_EVAL_CONF_BAD_LABELS : ROVIT_EVAL_CONF_N_LABELLED], (unsigned long long)s_bad[tid]);
    }
  }
  if (tally && blockIdx.x == 0 && tid == 0) res[ROVIT_EVAL_CONF_N] = (unsigned long long)n;
}

// per _MU_SCALED score: the chunk sums of sigma, every thread its chunks in order, then one fixed tree
__global__ __launch_bounds__(NT) void conf_apply_final_kernel(const rovit_eval_conf a, const double* __restrict__ partials, int chunks) {
  __shared__ double s_d[4];
  const int per = 16 + 32 * a.num_levels;
  for (int m = blockIdx.x; m < a.num_scores; m += gridDim.x) {
    if (a.score_kind[m] != ROVIT_EVAL_CONF_MU_SCALED) continue;
    double t = 0.0;
    for (int c = threadIdx.x; c < chunks; c += NT) t += partials[(size_t)m * chunks + c];
    t = block_sum_t(t, s_d);
    if (threadIdx.x == 0) ((double*)a.result)[ROVIT_EVAL_CONF_APPLY_SCORES + (size_t)m * per + 2] = t;
  }
}

static inline bool limits_ok(int n, int M, int G, int A) {
  return n >= 1 && n <= ROVIT_EVAL_MAX_ROWS && M >= 1 && M <= MS && A >= 1 && A <= MA && G >= 1 && G <= 1 + MAXC;
}

// what the fit and the application check alike; 0 when the descriptor is sound
static int check_common(const rovit_eval_conf* p, const char* who, bool fit) {
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_EVAL_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_EVAL_MAX_ROWS);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= MAXC, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who, p->num_classes, MAXC);
  ROVIT_CHECK_ARG(p->num_scores >= 1 && p->num_scores <= MS, ROVIT_ERR_SHAPE, "%s: %d scores (1..%d)", who, p->num_scores, MS);
  ROVIT_CHECK_ARG(p->num_levels >= 1 && p->num_levels <= MA, ROVIT_ERR_SHAPE, "%s: %d levels (1..%d)", who, p->num_levels, MA);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->raps_k >= 0 && p->raps_k <= MAXC, ROVIT_ERR_SHAPE, "%s: raps_k %d (0..%d)", who, p->raps_k, MAXC);
  ROVIT_CHECK_ARG(p->raps_lambda >= 0.f && p->raps_lambda < __builtin_inff(), ROVIT_ERR_SHAPE, "%s: raps_lambda must be finite and >= 0", who);
  ROVIT_CHECK_ARG((unsigned long long)p->row_offset + (unsigned)p->n <= 0xFFFFFFFFull, ROVIT_ERR_SHAPE, "%s: row_offset + n passes 2^32", who);
  const bool labelled = fit || p->label;
  bool need_kan = false, need_mu = false, need_sigma = false;
  for (int m = 0; m < p->num_scores; ++m) {
    const int kind = p->score_kind[m];
    ROVIT_CHECK_ARG(kind >= ROVIT_EVAL_CONF_LAC && kind <= ROVIT_EVAL_CONF_COLUMN, ROVIT_ERR_SHAPE, "%s: score %d has the unknown kind %d", who, m, kind);
    ROVIT_CHECK_ARG(labelled || kind <= ROVIT_EVAL_CONF_RAPS, ROVIT_ERR_NULL, "%s: score %d needs the labels (null pointer)", who, m);
    ROVIT_CHECK_ARG(kind != ROVIT_EVAL_CONF_COLUMN || p->score_column[m], ROVIT_ERR_NULL, "%s: score %d is a column with a null pointer", who, m);
    ROVIT_CHECK_ARG(kind != ROVIT_EVAL_CONF_COLUMN || rovit_aligned(p->score_column[m], 4), ROVIT_ERR_ALIGN,
                    "%s: the column of score %d is not aligned to its element size", who, m);
    need_kan |= kind == ROVIT_EVAL_CONF_KAN_ABS;
    need_mu |= kind == ROVIT_EVAL_CONF_MU_ABS || kind == ROVIT_EVAL_CONF_MU_SCALED;
    need_sigma |= kind == ROVIT_EVAL_CONF_MU_SCALED;
  }
  ROVIT_CHECK_ARG(p->probs && (!fit || p->label) && (!need_kan || (p->sev_pred && p->sev_true)) && (!need_mu || (p->mu && p->sev_true)) &&
                      (!need_sigma || p->uncertainty),
                  ROVIT_ERR_NULL, "%s: a record array is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->probs) && rovit_aligned(p->label, 4) && rovit_aligned(p->sev_pred, 4) && rovit_aligned(p->sev_true, 4) &&
                      rovit_aligned(p->uncertainty, 4) && rovit_aligned(p->mu, 4),
                  ROVIT_ERR_ALIGN, "%s: a record array is not aligned (probs to 16 bytes, the columns to 4)", who);
  ROVIT_CHECK_ARG(!labelled || (p->workspace && p->result), ROVIT_ERR_NULL, "%s: the workspace or the result block is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->workspace) && rovit_aligned(p->result, 8), ROVIT_ERR_ALIGN, "%s: the workspace or the result block is not aligned",
                  who);
  return ROVIT_OK;
}

}  // namespace

extern "C" size_t rovit_eval_conformal_workspace_bytes(int n, int M, int G, int A) { return limits_ok(n, M, G, A) ? layout(n, M, G, A).total : 0; }

extern "C" int rovit_eval_conformal(const rovit_eval_conf* p, rovit_stream_t stream) {
  const char* who = "eval_conformal";
  const int rc = check_common(p, who, true);
  if (rc != ROVIT_OK) return rc;
  const int n = p->n, M = p->num_scores, A = p->num_levels, G = p->class_conditional ? 1 + p->num_classes : 1, E = M * G * A;
  for (int lvl = 0; lvl < A; ++lvl)
    ROVIT_CHECK_ARG(p->alpha_num[lvl] >= 1 && p->alpha_num[lvl] < p->alpha_den[lvl] && p->alpha_den[lvl] <= ROVIT_EVAL_CONF_MAX_DEN, ROVIT_ERR_SHAPE,
                    "%s: level %d is %u/%u (0 < num < den <= %u)", who, lvl, p->alpha_num[lvl], p->alpha_den[lvl], ROVIT_EVAL_CONF_MAX_DEN);
  ROVIT_CHECK_ARG(rovit_aligned(p->scores_out, 4) && rovit_aligned(p->u_out, 4), ROVIT_ERR_ALIGN, "%s: a matrix to leave behind is not aligned", who);
  const Layout l = layout(n, M, G, A);
  ROVIT_CHECK_ARG(p->workspace_bytes >= l.total, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes,
                  l.total);
  const size_t lds = ((size_t)G * A + (size_t)G * A * 256) * 4;
  ROVIT_CHECK_ARG(lds <= 64 * 1024 || rovit_set_max_lds((const void*)conf_hist_kernel, (size_t)(80 * 1024)), ROVIT_ERR_LAUNCH,
                  "%s: cannot raise the LDS limit", who);

  char* ws = (char*)p->workspace;
  Fit f;
  f.n = n; f.M = M; f.G = G; f.A = A; f.E = E;
  f.x = (const float*)(ws + l.x);
  f.flags = (const unsigned short*)(ws + l.flags);
  f.cnt = (const unsigned*)(ws + l.cnt);
  f.prefix = (unsigned*)(ws + l.prefix);
  f.krem = (unsigned*)(ws + l.krem);
  f.trivial = (unsigned*)(ws + l.trivial);
  f.hist = (unsigned*)(ws + l.hist);
  f.result = (long long*)p->result;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(ws + l.cnt, 0, l.total - l.cnt, s) != hipSuccess ||
      hipMemsetAsync(p->result, 0, ROVIT_EVAL_CONF_WORDS(M, G, A) * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  const long long cap = p->max_workgroups > 0 ? p->max_workgroups : (1ll << 30);
  auto grid = [&](long long items) { return dim3((unsigned)(items < cap ? items : cap)); };
  const int chunks = (n + NT - 1) / NT, hchunks = (n + NT * HR - 1) / (NT * HR);
  hipLaunchKernelGGL(conf_score_kernel, grid(chunks), dim3(NT), 0, s, *p, (float*)(ws + l.x), (unsigned short*)(ws + l.flags),
                     (unsigned*)(ws + l.cnt), chunks);
  ROVIT_CHECK_LAUNCH("conf_score_kernel");
  hipLaunchKernelGGL(conf_init_kernel, grid((E + NT - 1) / NT), dim3(NT), 0, s, *p, f);
  ROVIT_CHECK_LAUNCH("conf_init_kernel");
  for (int round = 0; round < 4; ++round) {
    hipLaunchKernelGGL(conf_hist_kernel, grid((long long)hchunks * M), dim3(NT), lds, s, f, round, hchunks);
    ROVIT_CHECK_LAUNCH("conf_hist_kernel");
    hipLaunchKernelGGL(conf_step_kernel, grid(E), dim3(64), 0, s, f, round);
    ROVIT_CHECK_LAUNCH("conf_step_kernel");
  }
  return ROVIT_OK;
}

extern "C" size_t rovit_eval_conformal_apply_workspace_bytes(int n, int M) {
  return limits_ok(n, M, 1, 1) ? rovit_up16((size_t)M * ((n + NT - 1) / NT) * 8) : 0;
}

extern "C" int rovit_eval_conformal_apply(const rovit_eval_conf* p, rovit_stream_t stream) {
  const char* who = "eval_conformal_apply";
  const int rc = check_common(p, who, false);
  if (rc != ROVIT_OK) return rc;
  const int n = p->n, M = p->num_scores, A = p->num_levels, G = p->class_conditional ? 1 + p->num_classes : 1;
  ROVIT_CHECK_ARG(p->thresholds, ROVIT_ERR_NULL, "%s: the thresholds are missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->thresholds, 4), ROVIT_ERR_ALIGN, "%s: the thresholds are not aligned", who);
  ROVIT_CHECK_ARG(p->label || p->member_out, ROVIT_ERR_NULL, "%s: neither labels nor a membership matrix: nothing to do (null pointer)", who);
  const bool tally = p->label != nullptr;
  const size_t need = rovit_up16((size_t)M * ((n + NT - 1) / NT) * 8);
  ROVIT_CHECK_ARG(!tally || p->workspace_bytes >= need, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who,
                  p->workspace_bytes, need);
  int Mcls = 0;
  for (int m = 0; m < M; ++m) Mcls += p->score_kind[m] <= ROVIT_EVAL_CONF_RAPS;
  hipStream_t s = (hipStream_t)stream;
  if (tally && hipMemsetAsync(p->result, 0, ROVIT_EVAL_CONF_APPLY_WORDS(M, A) * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  const long long cap = p->max_workgroups > 0 ? p->max_workgroups : (1ll << 30);
  auto grid = [&](long long items) { return dim3((unsigned)(items < cap ? items : cap)); };
  const int chunks = (n + NT - 1) / NT;
  const size_t lds = (size_t)M * (16 + 32 * A) * 4;
  hipLaunchKernelGGL(conf_apply_kernel, grid(chunks), dim3(NT), lds, s, *p, (double*)p->workspace, chunks, G, Mcls);
  ROVIT_CHECK_LAUNCH("conf_apply_kernel");
  if (tally) {
    hipLaunchKernelGGL(conf_apply_final_kernel, grid(M), dim3(NT), 0, s, *p, (const double*)p->workspace, chunks);
    ROVIT_CHECK_LAUNCH("conf_apply_final_kernel");
  }
  return ROVIT_OK;
}
