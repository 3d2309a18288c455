// Non-parametric bootstrap of the evaluation score card on the device (rovit_eval_bootstrap): R resamples of the accumulator's record
// arrays, each reduced to the finalise's result block and to a row of metrics, with no sort and no host round trip.
//
// What it adds to the reference: experiments/ablation.py (get_component_importance, the "delta Acc" column) compares point estimates
// of evaluation/metrics.py between two trained models and reports neither an interval nor a test; the percentile bootstrap (Efron &
// Tibshirani 1993) supplies both, and needs one full score card per resample.
//
// One workgroup per replicate, persistent over r = blockIdx.x, += gridDim.x.
//   draws   Philox4x32-10 (philox.h), key = seed, counter = (j / 4, r, ROVIT_EVAL_BOOT_STREAM, 0); word j % 4 gives idx = (word * n) >> 32.  A thread
//           owns quads q = tid, tid + BT, ...: one Philox call serves four draws, and pass 2 calls it again instead of storing them.
//   pass 1  gathers the rows; integer histograms (confusion matrix, calibration bins, non-finite, bad labels) and the two rank
//           histograms H_a, H_b [less[idx]] += 1 through integer atomics; Brier and |severity error| as fp64 sums private to a thread in
//           its own draw order, folded by a fixed tree; the per-bin confidences per wave: for each bin that occurs among the wave's 64
//           draws, one fixed xor-tree sum, added by lane 0 to the wave's own accumulator.  No floating-point atomic anywhere: every
//           floating sum is a function of (records, seed, r, n, BT) and of nothing else -- not of the grid, not of where H lives.
//   scan    less[i] = #{x_j < x_i} is the start slot of row i's tie group in sorted order, so with P the exclusive prefix sum of H the
//           doubled tie-averaged rank of a draw inside the resample is 2 P[v] + H[v] + 1, v = less[idx]: H is overwritten by that rank.
//   pass 2  the same draws again: the three int64 rank sums.
// H lives in LDS up to ROVIT_EVAL_BOOT_LDS_ROWS rows (2 n words of dynamic LDS, so small sets leave room for several workgroups per CU),
// above it in the workgroup's slice of the caller's workspace.  There it is touched with agent-scope relaxed atomics only, loads and
// stores included: the adds are performed in L2, and a plain load could be served from a stale line of the CU's vector cache.
// Every index that reaches memory is clamped (draw, less value, predicted class, stratification tables), so no record content can
// send a thread out of bounds.
#include "common.h"
#include "philox.h"

namespace {

constexpr int EC = ROVIT_EVAL_MAX_CLASSES, EB = ROVIT_EVAL_MAX_BINS;
constexpr int BT = 512, BW = BT / 64;       // threads and waves per workgroup
constexpr int NH = 3 * 64 + 3;              // counters, as in evaluate.hip: confusion | bin count | bin correct | non-finite a, b | bad labels
constexpr int LDS_GRID = 1024;              // workgroups at most while H is in LDS (four per CU)

template <bool G> __device__ __forceinline__ unsigned h_load(const unsigned* p) {
  if (G) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}
template <bool G> __device__ __forceinline__ void h_store(unsigned* p, unsigned v) {
  if (G) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
// phase boundary of H: in the workspace the agent-scope fence waits for the outstanding stores and adds before the barrier
template <bool G> __device__ __forceinline__ void h_sync() {
  if (G) __threadfence();
  __syncthreads();
}
template <bool G> __device__ __forceinline__ void h_inc(unsigned* p) {
  if (G) __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else atomicAdd(p, 1u);
}

// the row of draw j of replicate r from its Philox word
__device__ __forceinline__ int draw_row(const rovit_eval_boot& a, const int* s_starts, int j, unsigned word) {
  const int n = a.n;
  int i;
  if (a.perm) {
    const int S = a.num_classes + 1;                      // segments: one per class, then the bad labels
    int s = 0;
    for (int k = 1; k < S; ++k) s = j >= s_starts[k] ? k : s;
    const int lo = s_starts[s], nc = max(s_starts[s + 1] - lo, 1);
    const int k = min(max(lo + (int)(((unsigned long long)word * (unsigned)nc) >> 32), 0), n - 1);
    i = a.perm[k];
  } else {
    i = (int)(((unsigned long long)word * (unsigned)n) >> 32);
  }
  return min(max(i, 0), n - 1);
}

template <bool G>
__global__ __launch_bounds__(BT) void eval_bootstrap_kernel(const rovit_eval_boot a) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_dyn[];
  __shared__ unsigned s_hist[NH];
  __shared__ double s_edges[EB + 1];
  __shared__ double s_conf[BW][EB];
  __shared__ double s_d[BW];
  __shared__ long long s_l[BW];
  __shared__ unsigned s_scan[2][BW];
  __shared__ unsigned s_carry[2];
  __shared__ int s_starts[EC + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n, C = a.num_classes, nb = a.n_bins;
  unsigned* Ha = G ? a.workspace + (size_t)blockIdx.x * 2 * (size_t)n : s_dyn;
  unsigned* Hb = Ha + n;
  const unsigned* less_a = a.rank_counts;
  const unsigned* less_b = a.rank_counts + 2 * (size_t)n;
  if (tid <= nb) s_edges[tid] = a.bin_edges[tid];
  if (a.perm && tid < C + 2) s_starts[tid] = min(max(a.starts[tid], 0), n);
  const int quads = (n + 3) >> 2;

  for (int r = blockIdx.x; r < a.num_resamples; r += gridDim.x) {
    __syncthreads();                                      // the previous replicate's readers are done
    if (tid < NH) s_hist[tid] = 0;
    for (int k = tid; k < BW * EB; k += BT) (&s_conf[0][0])[k] = 0.0;
    for (int k = tid; k < 2 * n; k += BT) h_store<G>(Ha + k, 0u);
    h_sync<G>();

    // ---- pass 1 ----
    double brier = 0.0, aerr = 0.0;
    for (int q0 = 0; q0 < quads; q0 += BT) {              // uniform trip count: the wave sums below need every lane
      const int q = q0 + tid;
      U4 w4 = {0u, 0u, 0u, 0u};
      if (q < quads) w4 = philox4x32_10(a.seed, (unsigned)q, (unsigned)r, ROVIT_EVAL_BOOT_STREAM, 0u);
      const unsigned words[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = 4 * q + e;
        int bin = -1;
        double conf = 0.0;
        if (q < quads && j < n) {
          const int i = draw_row(a, s_starts, j, words[e]);
          const int t = a.label[i];
          const int p = min(max(a.pred[i], 0), C - 1);
          double b = 0.0;
          for (int c = 0; c < C; ++c) {
            const double pc = (double)a.probs[(size_t)i * C + c];
            const double d = pc - (c == t ? 1.0 : 0.0);
            b += d * d;
            if (c == p) conf = pc;
          }
          brier += b;
          for (int k = 0; k < nb; ++k)
            if (conf > s_edges[k] && conf <= s_edges[k + 1]) bin = k;         // metrics.py:53, on doubles
          if (t >= 0 && t < C) atomicAdd(&s_hist[t * C + p], 1u); else atomicAdd(&s_hist[194], 1u);
          if (bin >= 0) {
            atomicAdd(&s_hist[64 + bin], 1u);
            if (p == t) atomicAdd(&s_hist[128 + bin], 1u);
          }
          const float st = a.sev_true[i], sp = a.sev_pred[i];
          aerr += fabs((double)st - (double)sp);
          if (!isfinite(st)) atomicAdd(&s_hist[192], 1u);
          if (!isfinite(sp)) atomicAdd(&s_hist[193], 1u);
          h_inc<G>(Ha + min(less_a[i], (unsigned)(n - 1)));
          h_inc<G>(Hb + min(less_b[i], (unsigned)(n - 1)));
        }
        // per-bin confidence: one fixed-tree wave sum per bin that occurs among these 64 draws, in lane order of first occurrence
        unsigned long long todo = __ballot(bin >= 0);
        while (todo) {
          const int k = __shfl(bin, __ffsll((long long)todo) - 1);
          const bool mine = bin == k;
          const double s = wave_sum_t(mine ? conf : 0.0);
          if (lane == 0) s_conf[wave][k] += s;
          todo &= ~__ballot(mine);
        }
      }
    }
    h_sync<G>();                                          // H, s_hist and s_conf complete
    const double sum_brier = block_sum_t<BW>(brier, s_d);
    const double sum_aerr = block_sum_t<BW>(aerr, s_d);

    // ---- scan: H[v] <- 2 P[v] + H[v] + 1 ----
    if (tid < 2) s_carry[tid] = 0;
    __syncthreads();
    for (int v0 = 0; v0 < n; v0 += BT) {
      const int v = v0 + tid;
      const unsigned ha = v < n ? h_load<G>(Ha + v) : 0u, hb = v < n ? h_load<G>(Hb + v) : 0u;
      unsigned ia = ha, ib = hb;                          // inclusive scan inside the wave
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        const unsigned ua = __shfl_up(ia, m), ub = __shfl_up(ib, m);
        if (lane >= m) { ia += ua; ib += ub; }
      }
      if (lane == 63) { s_scan[0][wave] = ia; s_scan[1][wave] = ib; }
      __syncthreads();
      unsigned pa = s_carry[0], pb = s_carry[1], ta = 0, tb = 0;
#pragma unroll
      for (int w = 0; w < BW; ++w) {
        if (w < wave) { pa += s_scan[0][w]; pb += s_scan[1][w]; }
        ta += s_scan[0][w]; tb += s_scan[1][w];
      }
      if (v < n) {
        h_store<G>(Ha + v, 2u * (pa + ia - ha) + ha + 1u);
        h_store<G>(Hb + v, 2u * (pb + ib - hb) + hb + 1u);
      }
      __syncthreads();                                    // everyone has read s_carry and s_scan
      if (tid == 0) { s_carry[0] += ta; s_carry[1] += tb; }
    }
    h_sync<G>();

    // ---- pass 2 ----
    long long rab = 0, raa = 0, rbb = 0;
    for (int q = tid; q < quads; q += BT) {
      const U4 w4 = philox4x32_10(a.seed, (unsigned)q, (unsigned)r, ROVIT_EVAL_BOOT_STREAM, 0u);
      const unsigned words[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = 4 * q + e;
        if (j < n) {
          const int i = draw_row(a, s_starts, j, words[e]);
          const long long da = (long long)h_load<G>(Ha + min(less_a[i], (unsigned)(n - 1))) - (n + 1);
          const long long db = (long long)h_load<G>(Hb + min(less_b[i], (unsigned)(n - 1))) - (n + 1);
          rab += da * db; raa += da * da; rbb += db * db;
        }
      }
    }
    rab = block_sum_t<BW>(rab, s_l);
    raa = block_sum_t<BW>(raa, s_l);
    rbb = block_sum_t<BW>(rbb, s_l);
    const bool finite = s_hist[192] == 0 && s_hist[193] == 0;
    if (!finite) rab = raa = rbb = 0;                     // the host restatement's convention: no rank sums beside a non-finite value

    // ---- outputs ----
    if (a.blocks) {
      long long* blk = (long long*)a.blocks + (size_t)r * ROVIT_EVAL_RESULT_WORDS;
      double* fblk = (double*)blk;
      if (tid < 192) blk[tid] = s_hist[tid];
      if (tid < nb) {
        double s = s_conf[0][tid];
        for (int w = 1; w < BW; ++w) s += s_conf[w][tid];
        fblk[ROVIT_EVAL_BIN_CONF + tid] = s;
      }
      // the words nothing else writes: padding, bins beyond n_bins, the loss sums
      if (tid == ROVIT_EVAL_N + 1 || (tid >= ROVIT_EVAL_BIN_CONF + nb && tid < ROVIT_EVAL_BRIER) ||
          (tid >= ROVIT_EVAL_LOSS && tid < ROVIT_EVAL_RESULT_WORDS))
        blk[tid] = 0;
      if (tid == 0) {
        blk[ROVIT_EVAL_RANK + 0] = rab; blk[ROVIT_EVAL_RANK + 1] = raa; blk[ROVIT_EVAL_RANK + 2] = rbb;
        blk[ROVIT_EVAL_NONFINITE + 0] = s_hist[192]; blk[ROVIT_EVAL_NONFINITE + 1] = s_hist[193];
        blk[ROVIT_EVAL_BAD_LABELS] = s_hist[194];
        blk[ROVIT_EVAL_N] = n;
        fblk[ROVIT_EVAL_BRIER] = sum_brier;
        fblk[ROVIT_EVAL_ABS_ERR] = sum_aerr;
      }
    }
    if (tid == 0) {
      // the arithmetic of metrics_from_block / prf_from_confusion / f1_averages (rovit_hip/evaluation.py), in fp64
      double* row = a.table + (size_t)r * ROVIT_EVAL_BOOT_COLS;
      const double dn = (double)n;
      double trace = 0.0, f1_sum = 0.0, wf1 = 0.0, support_sum = 0.0;
      int present = 0;
      for (int c = 0; c < EC; ++c) {
        double prec = 0.0, rec = 0.0, f1 = 0.0;
        if (c < C) {
          double pred_n = 0.0, true_n = 0.0;
          for (int k = 0; k < C; ++k) { pred_n += (double)s_hist[k * C + c]; true_n += (double)s_hist[c * C + k]; }
          const double tp = (double)s_hist[c * C + c];
          prec = pred_n > 0.0 ? tp / pred_n : 0.0;
          rec = true_n > 0.0 ? tp / true_n : 0.0;
          f1 = pred_n + true_n > 0.0 ? 2.0 * tp / (pred_n + true_n) : 0.0;
          if (pred_n + true_n > 0.0) { f1_sum += f1; ++present; }
          wf1 += f1 * true_n;
          support_sum += true_n;
          trace += tp;
        }
        row[ROVIT_EVAL_BOOT_PRECISION + c] = prec * 100.0;
        row[ROVIT_EVAL_BOOT_RECALL + c] = rec * 100.0;
        row[ROVIT_EVAL_BOOT_F1 + c] = f1 * 100.0;
      }
      double ece = 0.0;
      for (int k = 0; k < nb; ++k) {
        const double cnt = (double)s_hist[64 + k];
        if (cnt > 0.0) {
          double s = s_conf[0][k];
          for (int w = 1; w < BW; ++w) s += s_conf[w][k];
          ece += fabs(s / cnt - (double)s_hist[128 + k] / cnt) * (cnt / dn);
        }
      }
      row[ROVIT_EVAL_BOOT_ACCURACY] = trace / dn * 100.0;
      row[ROVIT_EVAL_BOOT_MACRO_F1] = (present ? f1_sum / (double)present : 0.0) * 100.0;
      row[ROVIT_EVAL_BOOT_WEIGHTED_F1] = (support_sum > 0.0 ? wf1 / support_sum : 0.0) * 100.0;
      row[ROVIT_EVAL_BOOT_MAE] = sum_aerr / dn;
      row[ROVIT_EVAL_BOOT_RHO] = finite && raa > 0 && rbb > 0 ? (double)rab / (sqrt((double)raa) * sqrt((double)rbb)) : __builtin_nan("");
      row[ROVIT_EVAL_BOOT_BRIER] = sum_brier / dn;
      row[ROVIT_EVAL_BOOT_ECE] = ece;
      row[ROVIT_EVAL_BOOT_COLS - 1] = 0.0;
    }
  }
}

static inline int ws_grid(int R, int cap) {
  int g = R < ROVIT_EVAL_BOOT_WORKSPACE_GRID ? R : ROVIT_EVAL_BOOT_WORKSPACE_GRID;
  return cap > 0 && cap < g ? cap : g;
}

}  // namespace

extern "C" size_t rovit_eval_bootstrap_workspace_bytes(int n, int num_resamples) {
  if (n <= ROVIT_EVAL_BOOT_LDS_ROWS || num_resamples < 1) return 0;
  return (size_t)ws_grid(num_resamples, 0) * 2 * (size_t)n * sizeof(unsigned);
}

extern "C" int rovit_eval_bootstrap(const rovit_eval_boot* p, rovit_stream_t stream) {
  const char* who = "eval_bootstrap";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= EC, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who, p->num_classes, EC);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_EVAL_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d recorded rows (1..%d, the finalise's limit)", who, p->n,
                  ROVIT_EVAL_MAX_ROWS);
  ROVIT_CHECK_ARG(p->n_bins >= 1 && p->n_bins <= EB, ROVIT_ERR_SHAPE, "%s: %d calibration bins (1..%d)", who, p->n_bins, EB);
  ROVIT_CHECK_ARG(p->num_resamples >= 1 && p->num_resamples <= ROVIT_EVAL_BOOT_MAX_RESAMPLES, ROVIT_ERR_SHAPE, "%s: %d resamples (1..%d)", who,
                  p->num_resamples, ROVIT_EVAL_BOOT_MAX_RESAMPLES);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (0: the default, or a positive cap)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->probs && p->pred && p->label && p->sev_pred && p->sev_true, ROVIT_ERR_NULL, "%s: a record array is missing (null pointer)",
                  who);
  ROVIT_CHECK_ARG(p->bin_edges && p->rank_counts && p->table, ROVIT_ERR_NULL,
                  "%s: bin edges, the finalise's rank counts or the metric table is missing (null pointer)", who);
  ROVIT_CHECK_ARG((p->perm == nullptr) == (p->starts == nullptr), ROVIT_ERR_NULL,
                  "%s: stratified resampling needs both the row permutation and the segment starts", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->probs) && rovit_aligned16(p->pred) && rovit_aligned16(p->label) && rovit_aligned16(p->sev_pred) &&
                      rovit_aligned16(p->sev_true),
                  ROVIT_ERR_ALIGN, "%s: a record array is not 16-byte aligned", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->bin_edges, 8) && rovit_aligned16(p->rank_counts) && rovit_aligned(p->table, 8) && rovit_aligned(p->blocks, 8) &&
                      rovit_aligned(p->perm, 4) && rovit_aligned(p->starts, 4) && rovit_aligned(p->workspace, 4),
                  ROVIT_ERR_ALIGN, "%s: bin edges, rank counts, a stratification table, the workspace or an output is not aligned", who);
  const int n = p->n, R = p->num_resamples;
  hipStream_t s = (hipStream_t)stream;
  if (n <= ROVIT_EVAL_BOOT_LDS_ROWS) {
    int grid = R < LDS_GRID ? R : LDS_GRID;
    if (p->max_workgroups > 0 && p->max_workgroups < grid) grid = p->max_workgroups;
    const size_t dyn = 2 * (size_t)n * sizeof(unsigned);
    if (dyn > 48 * 1024 &&
        hipFuncSetAttribute((const void*)eval_bootstrap_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) {
      (void)hipGetLastError();
      rovit_set_error("%s: the device refused %zu bytes of dynamic LDS", who, dyn);
      return ROVIT_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(eval_bootstrap_kernel<false>, dim3(grid), dim3(BT), dyn, s, *p);
  } else {
    const int grid = ws_grid(R, p->max_workgroups);
    const size_t need = (size_t)grid * 2 * (size_t)n * sizeof(unsigned);
    ROVIT_CHECK_ARG(p->workspace && p->workspace_bytes >= need, ROVIT_ERR_SHAPE,
                    "%s: %d rows exceed the LDS threshold of %d: the workspace must hold %zu bytes (rovit_eval_bootstrap_workspace_bytes), got %zu%s",
                    who, n, ROVIT_EVAL_BOOT_LDS_ROWS, need, p->workspace ? p->workspace_bytes : (size_t)0, p->workspace ? "" : " (null)");
    hipLaunchKernelGGL(eval_bootstrap_kernel<true>, dim3(grid), dim3(BT), 0, s, *p);
  }
  ROVIT_CHECK_LAUNCH("eval_bootstrap_kernel");
  return ROVIT_OK;
}
