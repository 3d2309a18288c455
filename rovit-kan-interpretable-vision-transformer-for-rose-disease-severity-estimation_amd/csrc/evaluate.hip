// Test-set evaluation and validation on the device: per-batch record (rovit_eval_accumulate) and per-epoch reduction
// (rovit_eval_finalize).
//
// Reference being replaced: evaluation/evaluator.py:37-67 (softmax, argmax, squeeze, exp and five device-to-host copies per
// batch), training/trainer.py:183-231 (six .item() per batch) and the sklearn / scipy calls of evaluation/metrics.py:9-61,96-122.
//
// accumulate: one thread per sample, C <= 8 logits in registers.  Everything it writes is a function of its own row, so the record
//   is deterministic by construction.
// finalize: three kernels on the caller's stream behind two memset nodes (the rank counts and the WHOLE result block, so that words no
//   kernel writes -- bins beyond n_bins, padding -- are zero and two result blocks can be compared byte for byte).
//   eval_rank_count_kernel  each thread owns one x_i of both severity arrays; tiles of x_j are staged in LDS and every lane reads
//                           the same address (a broadcast: no bank conflict); #{x_j < x_i} and #{x_j == x_i} are uint32 counts,
//                           added with integer atomics because the j range is split over workgroups to fill the chip at small n.
//                           The padding of the last tile is NaN, which is neither below nor equal to anything.
//   eval_partial_kernel     one workgroup per 256-row chunk: integer histograms (confusion matrix, bin counts) through LDS and integer
//                           atomics, the exact int64 rank sums, and the chunk's fp64 sums in a fixed order.
//   eval_final_kernel       one workgroup adds the chunk partials (and the loss table's columns) in a fixed order.
// O(n^2) counting by choice: exact, order-free, no sort.  n = 2^20 is the bound that keeps sum (R - n - 1)^2 <= n^3 inside int64.
// rovit_eval_finalize_ex with ROVIT_RANK_SORT replaces eval_rank_count_kernel only: both severity columns are sorted (sort_rank.hip) and
//   every row's less and eq come from two binary searches in its column's sorted keys: the same four count rows, word for word.
#include "common.h"
#include "rank_count.h"
#include "sort_device.h"

namespace {

constexpr int EC = ROVIT_EVAL_MAX_CLASSES, EB = ROVIT_EVAL_MAX_BINS;
constexpr int NT = 256;                 // threads per workgroup = rows per chunk
constexpr int PS = EB + 2;              // doubles per chunk partial: bin confidences, Brier, |severity error|
constexpr int NH = 3 * 64 + 3;          // LDS counters: confusion | bin count | bin correct | non-finite a, b | bad labels

__global__ __launch_bounds__(NT) void eval_accumulate_kernel(const rovit_eval_batch a) {
  if (a.losses && blockIdx.x == 0 && threadIdx.x < 5) a.loss_table[(size_t)a.loss_row * 5 + threadIdx.x] = a.losses[threadIdx.x];
  const int b = blockIdx.x * NT + threadIdx.x;
  if (b >= a.batch) return;
  const int C = a.num_classes;
  const size_t r = (size_t)a.offset + b;
  float z[EC];
  float zmax = -INFINITY;
#pragma unroll
  for (int j = 0; j < EC; ++j) {
    z[j] = j < C ? a.cls_logits[(size_t)b * C + j] : -INFINITY;
    zmax = fmaxf(zmax, z[j]);
  }
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < EC; ++j) {
    z[j] = j < C ? expf(z[j] - zmax) : 0.f;          // expf, not the fast intrinsic: the record is compared with torch.softmax
    se += z[j];
  }
  // first argmax of the fp32 probabilities; a NaN counts as the maximum, as in torch.argmax and np.argmax
  int best = 0;
  float bestv = z[0] / se;
#pragma unroll
  for (int j = 0; j < EC; ++j) {
    const float p = z[j] / se;
    if (j < C) {
      a.probs[r * C + j] = p;
      if (j > 0 && (p > bestv || (p != p && bestv == bestv))) { best = j; bestv = p; }
    }
  }
  a.pred[r] = best;
  const long long t = a.class_labels[b];
  a.label[r] = t >= 0 && t < C ? (int)t : -1;
  const float y = a.severity_is_int64 ? (float)((const long long*)a.severity_labels)[b] : ((const float*)a.severity_labels)[b];
  a.sev_true[r] = y;
  a.sev_pred[r] = a.kan_severity ? a.kan_severity[b] : y;                  // evaluator.py:50-53
  a.uncertainty[r] = a.log_var ? expf(0.5f * a.log_var[b]) : __builtin_nanf("");
}

__global__ __launch_bounds__(NT) void eval_rank_count_kernel(const float* __restrict__ A, const float* __restrict__ Bv, int n,
                                                             int tiles_per_split, unsigned* __restrict__ cnt) {
  __shared__ __attribute__((aligned(16))) float sA[RANK_RT];
  __shared__ __attribute__((aligned(16))) float sB[RANK_RT];
  const int i = blockIdx.x * NT + threadIdx.x;
  const float ai = i < n ? A[i] : 0.f, bi = i < n ? Bv[i] : 0.f;
  unsigned la = 0, ea = 0, lb = 0, eb = 0;
  const int ntiles = (n + RANK_RT - 1) / RANK_RT;
  const int t0 = blockIdx.y * tiles_per_split, t1 = min(ntiles, t0 + tiles_per_split);
  for (int t = t0; t < t1; ++t) {
    __syncthreads();
    // rank_count.h's tile over both columns at once, written out: as two calls each it measured 2.4 % slower (65 536 rows), staging alone 1.5 %
    for (int k = threadIdx.x; k < RANK_RT; k += NT) {
      const int j = t * RANK_RT + k;
      sA[k] = j < n ? A[j] : __builtin_nanf("");
      sB[k] = j < n ? Bv[j] : __builtin_nanf("");
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < RANK_RT / 4; ++k) {
      const float4 a4 = reinterpret_cast<const float4*>(sA)[k], b4 = reinterpret_cast<const float4*>(sB)[k];
      la += (a4.x < ai) + (a4.y < ai) + (a4.z < ai) + (a4.w < ai);
      ea += (a4.x == ai) + (a4.y == ai) + (a4.z == ai) + (a4.w == ai);
      lb += (b4.x < bi) + (b4.y < bi) + (b4.z < bi) + (b4.w < bi);
      eb += (b4.x == bi) + (b4.y == bi) + (b4.z == bi) + (b4.w == bi);
    }
  }
  if (i < n) {
    atomicAdd(&cnt[i], la);
    atomicAdd(&cnt[(size_t)n + i], ea);
    atomicAdd(&cnt[2 * (size_t)n + i], lb);
    atomicAdd(&cnt[3 * (size_t)n + i], eb);
  }
}

__global__ __launch_bounds__(NT) void eval_partial_kernel(const rovit_eval_final a) {
  __shared__ unsigned s_hist[NH];
  __shared__ int s_bin[NT];
  __shared__ double s_conf[NT];
  __shared__ double s_d[4];
  __shared__ long long s_l[4];
  const int tid = threadIdx.x, C = a.num_classes, nb = a.n_bins, n = a.n;
  const int i = blockIdx.x * NT + tid;
  if (tid < NH) s_hist[tid] = 0;
  __syncthreads();
  int bin = -1;
  double conf = 0.0, brier = 0.0, aerr = 0.0;
  long long da = 0, db = 0;
  if (i < n) {
    const int t = a.label[i];
    const int p = min(max(a.pred[i], 0), C - 1);
    for (int c = 0; c < C; ++c) {
      const double pc = (double)a.probs[(size_t)i * C + c];
      const double d = pc - (c == t ? 1.0 : 0.0);
      brier += d * d;
      if (c == p) conf = pc;
    }
    for (int k = 0; k < nb; ++k)
      if (conf > a.bin_edges[k] && conf <= a.bin_edges[k + 1]) bin = k;         // metrics.py:53, on doubles
    if (t >= 0 && t < C) atomicAdd(&s_hist[t * C + p], 1u); else atomicAdd(&s_hist[194], 1u);
    if (bin >= 0) {
      atomicAdd(&s_hist[64 + bin], 1u);
      if (p == t) atomicAdd(&s_hist[128 + bin], 1u);
    }
    const float st = a.sev_true[i], sp = a.sev_pred[i];
    aerr = fabs((double)st - (double)sp);
    if (!isfinite(st)) atomicAdd(&s_hist[192], 1u);
    if (!isfinite(sp)) atomicAdd(&s_hist[193], 1u);
    const unsigned* cnt = a.rank_counts;
    da = 2ll * cnt[i] + cnt[(size_t)n + i] + 1 - (n + 1);
    db = 2ll * cnt[2 * (size_t)n + i] + cnt[3 * (size_t)n + i] + 1 - (n + 1);
  }
  s_bin[tid] = bin;
  s_conf[tid] = conf;
  double* part = a.partials + (size_t)blockIdx.x * PS;
  const double sb = block_sum_t(brier, s_d);
  const double sa = block_sum_t(aerr, s_d);
  const long long rab = block_sum_t(da * db, s_l), raa = block_sum_t(da * da, s_l), rbb = block_sum_t(db * db, s_l);
  unsigned long long* res = (unsigned long long*)a.result;
  if (tid == 0) {
    part[EB] = sb;
    part[EB + 1] = sa;
    atomicAdd(&res[ROVIT_EVAL_RANK + 0], (unsigned long long)rab);       // two's complement: the wrapped sum is the signed sum
    atomicAdd(&res[ROVIT_EVAL_RANK + 1], (unsigned long long)raa);
    atomicAdd(&res[ROVIT_EVAL_RANK + 2], (unsigned long long)rbb);
  }
  __syncthreads();                       // s_bin / s_conf / s_hist complete
  if (tid < nb) {
    double s = 0.0;
    for (int r = 0; r < NT; ++r) s += s_bin[r] == tid ? s_conf[r] : 0.0;      // row order: fixed
    part[tid] = s;
  }
  // counters 192..194 land on ROVIT_EVAL_NONFINITE + 0, + 1 and ROVIT_EVAL_BAD_LABELS
  if (tid < NH && s_hist[tid]) atomicAdd(&res[tid < 192 ? tid : ROVIT_EVAL_NONFINITE + (tid - 192)], (unsigned long long)s_hist[tid]);
}

__global__ __launch_bounds__(NT) void eval_final_kernel(const rovit_eval_final a, int chunks) {
  __shared__ double s_d[4];
  const int tid = threadIdx.x;
  double* res = (double*)a.result;
  for (int k = 0; k < a.n_bins + 2; ++k) {
    const int col = k < a.n_bins ? k : EB + (k - a.n_bins);
    double s = 0.0;
    for (int c = tid; c < chunks; c += NT) s += a.partials[(size_t)c * PS + col];
    s = block_sum_t(s, s_d);
    if (tid == 0) res[ROVIT_EVAL_BIN_CONF + col] = s;
  }
  for (int k = 0; k < 5; ++k) {
    double s = 0.0;
    for (int r = tid; r < a.n_loss_rows; r += NT) s += (double)a.loss_table[(size_t)r * 5 + k];
    s = block_sum_t(s, s_d);
    if (tid == 0) res[ROVIT_EVAL_LOSS + k] = s;
  }
  if (tid == 0) ((long long*)a.result)[ROVIT_EVAL_N] = a.n;
}

}  // namespace

extern "C" size_t rovit_eval_partials_doubles(int n) { return n > 0 ? (size_t)((n + NT - 1) / NT) * PS : 0; }

extern "C" int rovit_eval_accumulate(const rovit_eval_batch* p, rovit_stream_t stream) {
  const char* who = "eval_accumulate";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= EC, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who, p->num_classes, EC);
  ROVIT_CHECK_ARG(p->batch >= 1, ROVIT_ERR_SHAPE, "%s: batch %d (>= 1)", who, p->batch);
  ROVIT_CHECK_ARG(p->offset >= 0 && p->capacity >= 1 && p->capacity <= ROVIT_EVAL_MAX_ROWS && (long)p->offset + p->batch <= p->capacity,
                  ROVIT_ERR_SHAPE, "%s: rows [%d, %d + %d) do not fit the capacity %d (<= %d)", who, p->offset, p->offset, p->batch, p->capacity,
                  ROVIT_EVAL_MAX_ROWS);
  ROVIT_CHECK_ARG(p->cls_logits && p->class_labels && p->severity_labels, ROVIT_ERR_NULL, "%s: logits or labels missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->probs && p->pred && p->label && p->sev_pred && p->sev_true && p->uncertainty, ROVIT_ERR_NULL,
                  "%s: a record array is missing (null pointer)", who);
  ROVIT_CHECK_ARG(!p->losses || (p->loss_table && p->loss_row >= 0 && p->loss_row < p->loss_capacity), ROVIT_ERR_SHAPE,
                  "%s: loss row %d outside the loss table (%d rows%s)", who, p->loss_row, p->loss_capacity, p->loss_table ? "" : ", null");
  ROVIT_CHECK_ARG(rovit_aligned(p->cls_logits, 4) && rovit_aligned(p->kan_severity, 4) && rovit_aligned(p->log_var, 4) && rovit_aligned(p->losses, 4) &&
                      rovit_aligned(p->class_labels, 8) && rovit_aligned(p->severity_labels, p->severity_is_int64 ? 8 : 4),
                  ROVIT_ERR_ALIGN, "%s: an input pointer is not aligned to its element size", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->probs) && rovit_aligned16(p->pred) && rovit_aligned16(p->label) && rovit_aligned16(p->sev_pred) &&
                      rovit_aligned16(p->sev_true) && rovit_aligned16(p->uncertainty) && rovit_aligned(p->loss_table, 4),
                  ROVIT_ERR_ALIGN, "%s: a record array is not 16-byte aligned", who);
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3((p->batch + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, *p);
  ROVIT_CHECK_LAUNCH("eval_accumulate_kernel");
  return ROVIT_OK;
}

namespace {
// the rank workspace of the sorted finalise: the sorted keys and the permutations of sev_true and sev_pred, then the sort's own
struct FinalRankLayout { size_t keys, perm, sort, total; };
inline FinalRankLayout final_rank_layout(int n) {
  const int nn[2] = {n, n};
  FinalRankLayout l;
  l.keys = 0;
  l.perm = l.keys + 2 * rovit_up16((size_t)n * 4);
  l.sort = l.perm + 2 * rovit_up16((size_t)n * 4);
  l.total = l.sort + rovit_sort_batch_workspace_bytes(nn, 2);
  return l;
}
}  // namespace

extern "C" size_t rovit_eval_finalize_rank_workspace_bytes(int n) {
  return n >= 1 && n <= ROVIT_EVAL_MAX_ROWS ? final_rank_layout(n).total : 0;
}

extern "C" int rovit_eval_finalize(const rovit_eval_final* p, rovit_stream_t stream) {
  return rovit_eval_finalize_ex(p, ROVIT_RANK_COUNT, nullptr, 0, stream);
}

extern "C" int rovit_eval_finalize_ex(const rovit_eval_final* p, int method, void* rank_workspace, size_t rank_workspace_bytes,
                                      rovit_stream_t stream) {
  const char* who = "eval_finalize";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->num_classes >= 2 && p->num_classes <= EC, ROVIT_ERR_SHAPE, "%s: %d classes (2..%d)", who, p->num_classes, EC);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_EVAL_MAX_ROWS, ROVIT_ERR_SHAPE,
                  "%s: %d recorded rows (1..%d: the rank sums are exact in int64 up to there)", who, p->n, ROVIT_EVAL_MAX_ROWS);
  ROVIT_CHECK_ARG(p->n_bins >= 1 && p->n_bins <= EB, ROVIT_ERR_SHAPE, "%s: %d calibration bins (1..%d)", who, p->n_bins, EB);
  ROVIT_CHECK_ARG(p->n_loss_rows >= 0 && (p->n_loss_rows == 0 || p->loss_table), ROVIT_ERR_SHAPE, "%s: %d loss rows%s", who, p->n_loss_rows,
                  p->loss_table ? "" : " but no loss table");
  ROVIT_CHECK_ARG(p->probs && p->pred && p->label && p->sev_pred && p->sev_true, ROVIT_ERR_NULL, "%s: a record array is missing (null pointer)",
                  who);
  ROVIT_CHECK_ARG(p->bin_edges && p->rank_counts && p->partials && p->result, ROVIT_ERR_NULL,
                  "%s: bin edges, a workspace or the result block is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->probs) && rovit_aligned16(p->pred) && rovit_aligned16(p->label) && rovit_aligned16(p->sev_pred) &&
                      rovit_aligned16(p->sev_true) && rovit_aligned(p->loss_table, 4),
                  ROVIT_ERR_ALIGN, "%s: a record array is not 16-byte aligned", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->bin_edges, 8) && rovit_aligned16(p->rank_counts) && rovit_aligned(p->partials, 8) && rovit_aligned(p->result, 8),
                  ROVIT_ERR_ALIGN, "%s: bin edges, a workspace or the result block is not aligned", who);
  ROVIT_CHECK_ARG(method >= ROVIT_RANK_AUTO && method <= ROVIT_RANK_SORT, ROVIT_ERR_SHAPE, "%s: unknown rank method %d", who, method);
  const int n = p->n, chunks = (n + NT - 1) / NT, ntiles = (n + RANK_RT - 1) / RANK_RT;
  const bool sorted = rovit_rank_method(method, n) == ROVIT_RANK_SORT;
  const FinalRankLayout rl = final_rank_layout(n);
  if (sorted) {
    ROVIT_CHECK_ARG(rank_workspace, ROVIT_ERR_NULL, "%s: the rank workspace is missing (null pointer)", who);
    ROVIT_CHECK_ARG(rovit_aligned16(rank_workspace), ROVIT_ERR_ALIGN, "%s: the rank workspace is not 16-byte aligned", who);
    ROVIT_CHECK_ARG(rank_workspace_bytes >= rl.total, ROVIT_ERR_SHAPE, "%s: the rank workspace holds %zu bytes, %zu are needed", who,
                    rank_workspace_bytes, rl.total);
  }
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(p->rank_counts, 0, 4 * (size_t)n * sizeof(unsigned), s) != hipSuccess ||
      hipMemsetAsync(p->result, 0, ROVIT_EVAL_RESULT_WORDS * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  if (sorted) {
    // the same four count rows from two sorted columns: less and eq of every row by two binary searches in its own column's keys
    char* ws = (char*)rank_workspace;
    const size_t col = rovit_up16((size_t)n * 4);
    unsigned* keys[2] = {(unsigned*)(ws + rl.keys), (unsigned*)(ws + rl.keys + col)};
    unsigned* perm[2] = {(unsigned*)(ws + rl.perm), (unsigned*)(ws + rl.perm + col)};
    const RovitSortCol c[2] = {{p->sev_true, keys[0], perm[0], n}, {p->sev_pred, keys[1], perm[1], n}};
    int rc = rovit_sort_batch(c, 2, ws + rl.sort, rank_workspace_bytes - rl.sort, 0, s, who);
    if (rc != ROVIT_OK) return rc;
    const RovitRankQuery q[2] = {{p->sev_true, n, keys[0], n, p->rank_counts, p->rank_counts + (size_t)n},
                                 {p->sev_pred, n, keys[1], n, p->rank_counts + 2 * (size_t)n, p->rank_counts + 3 * (size_t)n}};
    rc = rovit_rank_search(q, 2, 0, s, who);
    if (rc != ROVIT_OK) return rc;
  } else {
    // split the j range until about 1024 workgroups exist (four per CU); the counts are integers, so the split changes nothing
    int splits = (1024 + chunks - 1) / chunks;
    splits = splits < 1 ? 1 : (splits > ntiles ? ntiles : splits);
    const int tps = (ntiles + splits - 1) / splits;
    splits = (ntiles + tps - 1) / tps;
    hipLaunchKernelGGL(eval_rank_count_kernel, dim3(chunks, splits), dim3(NT), 0, s, p->sev_true, p->sev_pred, n, tps, p->rank_counts);
    ROVIT_CHECK_LAUNCH("eval_rank_count_kernel");
  }
  hipLaunchKernelGGL(eval_partial_kernel, dim3(chunks), dim3(NT), 0, s, *p);
  ROVIT_CHECK_LAUNCH("eval_partial_kernel");
  hipLaunchKernelGGL(eval_final_kernel, dim3(1), dim3(NT), 0, s, *p, chunks);
  ROVIT_CHECK_LAUNCH("eval_final_kernel");
  return ROVIT_OK;
}
