// Post-hoc calibration on the device: one temperature for the classifier, one scale for the Gaussian head's sigma and the observed
// coverage of its central intervals, fitted on the accumulator's recorded rows (rovit_eval_calibrate), and the elementwise launch that
// applies them to a record (rovit_eval_recalibrate).  Definitions: include/rovit_hip.h; numpy restatement: rovit_hip/evaluation.py,
// calibration_reference.
//
// Reference being extended: evaluation/metrics.py reports ECE and the Brier score and nothing acts on them.
//
// Launches on the caller's stream behind one memset node (the WHOLE result block):
//   cal_reg_kernel        one thread per row: z^2 and ln sigma summed per 256-row chunk in a fixed tree, the row counters and the L
//                         coverage counts through wave ballots, LDS and integer atomics.  Skipped without a regression part.
//   cal_search_kernel<0>  per round: ONE CANDIDATE PER LANE.  A workgroup stages a 256-row chunk as fp64 l, the row maximum and the
//                         label in LDS; each of its four waves walks 64 of those rows, every lane reads the same LDS address (a
//                         broadcast: no bank conflict) and adds the row's term of g to its own candidate's fp64 sum.  No cross-lane
//                         reduction: the four waves are added in order, and the chunk's 64 sums go to partial[chunk][candidate].
//   cal_step_kernel<0>    one workgroup: the chunk partials in a fixed order (four contiguous runs, then those four in order), then
//                         the bracket rule on the device-resident state that the next round's launch reads.
//   cal_search_kernel<1>  the same row code at u = 0 (lane 0) and u = u* (lane 1), summing the row's NLL instead; counts the bad labels.
//   cal_step_kernel<1>    folds those and the regression partials and writes the block.
// A chunk is a function of n alone and a workgroup walks chunks with a stride of the grid: no partial depends on the grid.
#include "common.h"

namespace {

constexpr int NT = 256;                 // threads per workgroup = rows per chunk
constexpr int NC = ROVIT_EVAL_CAL_CANDIDATES;
constexpr int MC = ROVIT_EVAL_MAX_CLASSES, ML = ROVIT_EVAL_CAL_MAX_LEVELS;
static_assert(NC == 64, "one candidate per lane of a wave64");
static_assert(NT == 4 * NC, "four waves per chunk, folded in order");

struct State {                           // the search's bracket between launches
  double lo, hi, g_lo, g_hi, u;
  int done, status;
};

struct Args {
  int n, C, L, chunks;
  const float* probs; const int* label; const float* sev_true; const float* unc; const float* mu;
  const double* hw;
  State* state;
  double* partial;                       // (chunks, 64)
  double* regp;                          // (chunks, 2): sum z^2, sum ln sigma
  void* result;
};

// u_j of a bracket: one division, one multiplication, one addition, none of them contracted, so the numpy restatement gets the same bits
__device__ __forceinline__ double candidate(double lo, double hi, int j) {
#pragma clang fp contract(off)
  const double step = (hi - lo) * ((double)j / (double)(NC - 1));
  return j == NC - 1 ? hi : lo + step;
}
// lo - (hi - lo) g_lo / (g_hi - g_lo), uncontracted for the same reason; the ratio lies in [-1, 0] whenever g_lo < 0 <= g_hi, so
// subnormal g values cannot overflow it
__device__ __forceinline__ double secant(double lo, double hi, double g_lo, double g_hi) {
#pragma clang fp contract(off)
  const double t = (hi - lo) * (g_lo / (g_hi - g_lo));
  return lo - t;
}

__device__ __forceinline__ double log_prob(float p) { return fmax(log((double)p), ROVIT_EVAL_CAL_LOG_FLOOR); }

// one row at one beta: MODE 0 the row's term of g, sum_c w_c l_c - l_y; MODE 1 its NLL, logsumexp_c(beta l_c) - beta l_y
template <int MODE>
__device__ __forceinline__ double row_term(const double* __restrict__ l, int C, double lmax, int lab, double beta) {
  double s = 0.0, a = 0.0;
  for (int c = 0; c < C; ++c) {
    const double e = exp(beta * (l[c] - lmax));
    s += e;
    a += e * l[c];
  }
  return MODE == 0 ? a / s - l[lab] : beta * lmax + log(s) - beta * l[lab];
}

template <int MODE>
__global__ __launch_bounds__(NT) void cal_search_kernel(const Args a, int round) {
  __shared__ __attribute__((aligned(16))) double sL[NT * MC];
  __shared__ double sMax[NT];
  __shared__ double sFold[4][NC];
  __shared__ int sLab[NT];
  __shared__ unsigned sBad;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = a.n, C = a.C;
  double u;
  if (MODE == 0) {
    if (round > 0 && a.state->done) return;
    const double lo = round == 0 ? -ROVIT_EVAL_CAL_U_MAX : a.state->lo, hi = round == 0 ? ROVIT_EVAL_CAL_U_MAX : a.state->hi;
    u = candidate(lo, hi, lane);
  } else {
    u = lane == 1 ? a.state->u : 0.0;
  }
  const double beta = exp(u);
  if (tid == 0) sBad = 0;
  unsigned bad = 0;
  for (int w = blockIdx.x; w < a.chunks; w += gridDim.x) {
    __syncthreads();                                        // the previous chunk's readers are done
    const int i = w * NT + tid;
    int lab = -1;
    if (i < n) {
      lab = a.label[i];
      lab = lab >= 0 && lab < C ? lab : -1;
      bad += lab < 0;
      double m = ROVIT_EVAL_CAL_LOG_FLOOR;
      for (int c = 0; c < C; ++c) {
        const double v = log_prob(a.probs[(size_t)i * C + c]);
        sL[tid * C + c] = v;
        m = fmax(m, v);
      }
      sMax[tid] = m;
    }
    sLab[tid] = lab;
    __syncthreads();
    double acc = 0.0;
    for (int r = 0; r < NC; ++r) {
      const int row = wave * NC + r;                        // the same row in every lane
      const int y = sLab[row];
      if (y >= 0) acc += row_term<MODE>(sL + row * C, C, sMax[row], y, beta);
    }
    sFold[wave][lane] = acc;
    __syncthreads();
    if (tid < NC) a.partial[(size_t)w * NC + tid] = ((sFold[0][tid] + sFold[1][tid]) + sFold[2][tid]) + sFold[3][tid];
  }
  if (MODE == 1) {
    if (bad) atomicAdd(&sBad, bad);
    __syncthreads();
    if (tid == 0 && sBad) atomicAdd(&((unsigned long long*)a.result)[ROVIT_EVAL_CAL_BAD_LABELS], (unsigned long long)sBad);
  }
}

__global__ __launch_bounds__(NT) void cal_reg_kernel(const Args a) {
  __shared__ double s4[4];
  __shared__ double sHw[ML];
  __shared__ unsigned sCov[ML], sCnt[2];
  const int tid = threadIdx.x, lane = tid & 63, n = a.n, L = a.L;
  if (tid < L) sHw[tid] = a.hw[tid];
  for (int w = blockIdx.x; w < a.chunks; w += gridDim.x) {
    __syncthreads();
    if (tid < ML) sCov[tid] = 0;
    if (tid < 2) sCnt[tid] = 0;
    __syncthreads();
    const int i = w * NT + tid;
    bool valid = false;
    double d = 0.0, sg = 1.0;
    if (i < n) {
      sg = (double)a.unc[i];
      const double m = (double)a.mu[i], t = (double)a.sev_true[i];
      valid = isfinite(sg) && sg > 0.0 && isfinite(m) && isfinite(t);
      d = t - m;
    }
    const double z = valid ? d / sg : 0.0;
    const double z2 = z * z, ls = valid ? log(sg) : 0.0;
    const double ad = fabs(d);
    for (int k = 0; k < L; ++k) {
      const unsigned c = (unsigned)__popcll(__ballot(valid && ad <= sHw[k] * sg));
      if (lane == 0 && c) atomicAdd(&sCov[k], c);
    }
    const unsigned nv = (unsigned)__popcll(__ballot(valid)), nb = (unsigned)__popcll(__ballot(i < n && !valid));
    if (lane == 0) {
      if (nv) atomicAdd(&sCnt[0], nv);
      if (nb) atomicAdd(&sCnt[1], nb);
    }
    const double sz = block_sum_t<4>(z2, s4);
    const double sl = block_sum_t<4>(ls, s4);               // its first barrier also orders the LDS atomics above
    if (tid == 0) {
      a.regp[(size_t)w * 2] = sz;
      a.regp[(size_t)w * 2 + 1] = sl;
    }
    unsigned long long* res = (unsigned long long*)a.result;
    if (tid < L && sCov[tid]) atomicAdd(&res[ROVIT_EVAL_CAL_COVERAGE + tid], (unsigned long long)sCov[tid]);
    if (tid < 2 && sCnt[tid]) atomicAdd(&res[ROVIT_EVAL_CAL_N_REG + tid], (unsigned long long)sCnt[tid]);
  }
}

template <int MODE>
__global__ __launch_bounds__(NT) void cal_step_kernel(const Args a, int round, int has_reg) {
  __shared__ double sFold[4][NC];
  __shared__ double sG[NC];
  __shared__ double s4[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, chunks = a.chunks;
  if (MODE == 0 && round > 0 && a.state->done) return;
  {                                                         // chunk partials: four contiguous runs, each in order, then the four in order
    const int per = (chunks + 3) / 4;
    const int c0 = wave * per, c1 = min(chunks, c0 + per);
    double s = 0.0;
    for (int c = c0; c < c1; ++c) s += a.partial[(size_t)c * NC + lane];
    sFold[wave][lane] = s;
    __syncthreads();
    if (tid < NC) sG[tid] = ((sFold[0][tid] + sFold[1][tid]) + sFold[2][tid]) + sFold[3][tid];
    __syncthreads();
  }
  if (MODE == 0) {
    if (tid != 0) return;
    State st;
    const double lo = round == 0 ? -ROVIT_EVAL_CAL_U_MAX : a.state->lo, hi = round == 0 ? ROVIT_EVAL_CAL_U_MAX : a.state->hi;
    int first = -1;                                         // the first j >= 1 with g(u_j) >= 0
    for (int j = NC - 1; j >= 1; --j) first = sG[j] >= 0.0 ? j : first;
    st.done = 0;
    st.status = ROVIT_EVAL_CAL_INTERIOR;
    if (round == 0 && sG[0] >= 0.0) {
      st.done = 1; st.status = ROVIT_EVAL_CAL_AT_MAX;
      st.lo = st.hi = st.u = lo; st.g_lo = st.g_hi = sG[0];
    } else if (round == 0 && first < 0) {
      st.done = 1; st.status = ROVIT_EVAL_CAL_AT_MIN;
      st.lo = st.hi = st.u = hi; st.g_lo = st.g_hi = sG[NC - 1];
    } else {
      const int j = first < 0 ? NC - 1 : first;
      st.lo = candidate(lo, hi, j - 1); st.hi = candidate(lo, hi, j);
      st.g_lo = sG[j - 1]; st.g_hi = sG[j];
      st.u = st.lo;
      if (round == ROVIT_EVAL_CAL_ROUNDS - 1 && st.g_hi != st.g_lo)          // the secant point of the last bracket
        st.u = secant(st.lo, st.hi, st.g_lo, st.g_hi);
    }
    *a.state = st;
  } else {
    double sz = 0.0, sl = 0.0;
    if (has_reg) {                                          // regression partials: 256 contiguous runs in order, then a fixed tree
      const int per = (chunks + NT - 1) / NT;
      const int c0 = tid * per, c1 = min(chunks, c0 + per);
      for (int c = c0; c < c1; ++c) {
        sz += a.regp[(size_t)c * 2];
        sl += a.regp[(size_t)c * 2 + 1];
      }
      sz = block_sum_t<4>(sz, s4);
      sl = block_sum_t<4>(sl, s4);
    }
    if (tid != 0) return;
    long long* res = (long long*)a.result;
    double* f = (double*)a.result;
    const State st = *a.state;
    res[ROVIT_EVAL_CAL_N] = a.n;
    res[ROVIT_EVAL_CAL_N_VALID] = a.n - res[ROVIT_EVAL_CAL_BAD_LABELS];          // the NLL launch's atomics are complete: stream order
    res[ROVIT_EVAL_CAL_STATUS] = st.status;
    f[ROVIT_EVAL_CAL_U] = st.u;
    f[ROVIT_EVAL_CAL_NLL] = sG[0];
    f[ROVIT_EVAL_CAL_NLL_CAL] = sG[1];
    f[ROVIT_EVAL_CAL_G_LO] = st.g_lo;
    f[ROVIT_EVAL_CAL_G_HI] = st.g_hi;
    f[ROVIT_EVAL_CAL_U_LO] = st.lo;
    f[ROVIT_EVAL_CAL_U_HI] = st.hi;
    f[ROVIT_EVAL_CAL_SUM_Z2] = sz;
    f[ROVIT_EVAL_CAL_SUM_LOG_SIGMA] = sl;
  }
}

__global__ __launch_bounds__(NT) void recalibrate_kernel(const rovit_eval_recal a) {
  const int n = a.n, C = a.num_classes;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    double l[MC], m = ROVIT_EVAL_CAL_LOG_FLOOR, s = 0.0;
#pragma unroll
    for (int c = 0; c < MC; ++c)
      if (c < C) {
        l[c] = log_prob(a.probs[(size_t)i * C + c]);
        m = fmax(m, l[c]);
      }
#pragma unroll
    for (int c = 0; c < MC; ++c)
      if (c < C) {
        l[c] = exp(a.beta * (l[c] - m));
        s += l[c];
      }
#pragma unroll
    for (int c = 0; c < MC; ++c)
      if (c < C) a.probs_out[(size_t)i * C + c] = (float)(l[c] / s);
    if (a.uncertainty_out) a.uncertainty_out[i] = (float)(a.sigma_scale * (double)a.uncertainty[i]);
  }
}

static inline bool limits_ok(int n, int C) { return n >= 1 && n <= ROVIT_EVAL_MAX_ROWS && C >= 2 && C <= MC; }
struct Layout { size_t state, partial, regp, total; };
static inline Layout layout(int n) {
  const size_t chunks = ((size_t)n + NT - 1) / NT;
  Layout l;
  l.state = 0;
  l.partial = rovit_up16(sizeof(State));
  l.regp = l.partial + rovit_up16(chunks * NC * 8);
  l.total = l.regp + rovit_up16(chunks * 2 * 8);
  return l;
}

}  // namespace

extern "C" size_t rovit_eval_calibrate_workspace_bytes(int n, int C) { return limits_ok(n, C) ? layout(n).total : 0; }

extern "C" int rovit_eval_calibrate(const rovit_eval_cal* p, rovit_stream_t stream) {
  const char* who = "eval_calibrate";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_EVAL_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d recorded rows (1..%d)", who, p->n, ROVIT_EVAL_MAX_ROWS);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= MC, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who, p->num_classes, MC);
  ROVIT_CHECK_ARG(p->num_levels >= 0 && p->num_levels <= ML, ROVIT_ERR_SHAPE, "%s: %d coverage levels (0..%d)", who, p->num_levels, ML);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->probs && p->label, ROVIT_ERR_NULL, "%s: a record array is missing (null pointer)", who);
  ROVIT_CHECK_ARG((p->mu != nullptr) == (p->uncertainty != nullptr), ROVIT_ERR_NULL,
                  "%s: the regression part needs both mu and uncertainty, or neither", who);
  const bool has_reg = p->mu != nullptr;
  ROVIT_CHECK_ARG(!has_reg || p->sev_true, ROVIT_ERR_NULL, "%s: the regression part needs sev_true (null pointer)", who);
  ROVIT_CHECK_ARG(!has_reg || p->num_levels == 0 || p->half_widths, ROVIT_ERR_NULL, "%s: the half-widths are missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->workspace && p->result, ROVIT_ERR_NULL, "%s: the workspace or the result block is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->probs) && rovit_aligned16(p->label) && rovit_aligned16(p->sev_true) && rovit_aligned16(p->uncertainty),
                  ROVIT_ERR_ALIGN, "%s: a record array is not 16-byte aligned", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->mu, 4) && rovit_aligned(p->half_widths, 8) && rovit_aligned16(p->workspace) && rovit_aligned(p->result, 8),
                  ROVIT_ERR_ALIGN, "%s: mu, the half-widths, the workspace or the result block is not aligned", who);
  const Layout l = layout(p->n);
  ROVIT_CHECK_ARG(p->workspace_bytes >= l.total, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes,
                  l.total);

  char* ws = (char*)p->workspace;
  Args a;
  a.n = p->n; a.C = p->num_classes; a.L = has_reg ? p->num_levels : 0; a.chunks = (p->n + NT - 1) / NT;
  a.probs = p->probs; a.label = p->label; a.sev_true = p->sev_true; a.unc = p->uncertainty; a.mu = p->mu; a.hw = p->half_widths;
  a.state = (State*)(ws + l.state);
  a.partial = (double*)(ws + l.partial);
  a.regp = (double*)(ws + l.regp);
  a.result = p->result;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(p->result, 0, ROVIT_EVAL_CAL_WORDS(p->num_levels) * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  const int cap = p->max_workgroups > 0 ? p->max_workgroups : (1 << 30);
  const dim3 grid((unsigned)(a.chunks < cap ? a.chunks : cap));
  if (has_reg) {
    hipLaunchKernelGGL(cal_reg_kernel, grid, dim3(NT), 0, s, a);
    ROVIT_CHECK_LAUNCH("cal_reg_kernel");
  }
  for (int r = 0; r < ROVIT_EVAL_CAL_ROUNDS; ++r) {
    hipLaunchKernelGGL(cal_search_kernel<0>, grid, dim3(NT), 0, s, a, r);
    ROVIT_CHECK_LAUNCH("cal_search_kernel");
    hipLaunchKernelGGL(cal_step_kernel<0>, dim3(1), dim3(NT), 0, s, a, r, 0);
    ROVIT_CHECK_LAUNCH("cal_step_kernel");
  }
  hipLaunchKernelGGL(cal_search_kernel<1>, grid, dim3(NT), 0, s, a, 0);
  ROVIT_CHECK_LAUNCH("cal_search_kernel (NLL)");
  hipLaunchKernelGGL(cal_step_kernel<1>, dim3(1), dim3(NT), 0, s, a, 0, (int)has_reg);
  ROVIT_CHECK_LAUNCH("cal_step_kernel (NLL)");
  return ROVIT_OK;
}

extern "C" int rovit_eval_recalibrate(const rovit_eval_recal* p, rovit_stream_t stream) {
  const char* who = "eval_recalibrate";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_EVAL_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d recorded rows (1..%d)", who, p->n, ROVIT_EVAL_MAX_ROWS);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= MC, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who, p->num_classes, MC);
  ROVIT_CHECK_ARG(p->beta > 0.0 && p->beta < 1e300 && p->sigma_scale > 0.0 && p->sigma_scale < 1e300, ROVIT_ERR_SHAPE,
                  "%s: beta %g and sigma_scale %g must be positive and finite", who, p->beta, p->sigma_scale);
  ROVIT_CHECK_ARG(p->probs && p->probs_out, ROVIT_ERR_NULL, "%s: probs or probs_out is missing (null pointer)", who);
  ROVIT_CHECK_ARG((p->uncertainty != nullptr) == (p->uncertainty_out != nullptr), ROVIT_ERR_NULL,
                  "%s: uncertainty and uncertainty_out go together", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->probs, 4) && rovit_aligned(p->probs_out, 4) && rovit_aligned(p->uncertainty, 4) && rovit_aligned(p->uncertainty_out, 4),
                  ROVIT_ERR_ALIGN, "%s: an array is not aligned to its element size", who);
  const int blocks = (p->n + NT - 1) / NT;
  hipLaunchKernelGGL(recalibrate_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, *p);
  ROVIT_CHECK_LAUNCH("recalibrate_kernel");
  return ROVIT_OK;
}
