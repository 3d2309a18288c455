// A training epoch with one synchronisation: the CutMix / MixUp loss in one launch (rovit_joint_loss_mixed) with a per-batch
// record, and the per-epoch reduction of that record (rovit_train_finalize).
//
// Reference being replaced: training/trainer.py:104-111 (the loss twice on the same head outputs and 15 element-wise launches
// that mix the five dict entries), :144-153 (five loss .item(), max / eq / sum and a sixth .item() per step) and :172-179.
//
// joint_loss_mixed_kernel has joint_loss_kernel's shape (one workgroup of 256 threads walks the batch) and its arithmetic: both
// call joint_loss::row and joint_loss::reduce of joint_loss_row.h.  Only the focal term depends on the class label, so
// lam L(a) + (1 - lam) L(b) is the same single pass with a second label column.  Thread 0 writes the batch's row of the epoch
// table; the host hands out the row index, so a row has one writer and the table needs neither a counter nor an atomic.
// train_final_kernel adds the rows in a fixed order (strided per thread, then the fixed tree of common.h's block_sum_t) in fp64.
#include "common.h"
#include "joint_loss_row.h"

namespace {

using joint_loss::LossArgs;
using joint_loss::MAXC;

constexpr int NT = 256;
constexpr int RW = ROVIT_TRAIN_ROW_WORDS;

struct MixedArgs {
  LossArgs l;
  const long long* cls_t_b;      // second label column or NULL
  float lam;
  unsigned* table;               // (capacity, RW) 4-byte words or NULL
  int row;
};

__global__ __launch_bounds__(NT) void joint_loss_mixed_kernel(const MixedArgs m) {
  __shared__ float s_red[4];
  __shared__ int s_cnt[4];
  const LossArgs& a = m.l;
  const float invB = 1.f / a.B;
  float l_cls = 0.f, l_ord = 0.f, l_unc = 0.f, l_kan = 0.f;
  int correct = 0;
  if (m.cls_t_b) {
    for (int b = threadIdx.x; b < a.B; b += NT) correct += joint_loss::row<true, true>(a, m.cls_t_b, m.lam, b, invB, l_cls, l_ord, l_unc, l_kan);
  } else {
    for (int b = threadIdx.x; b < a.B; b += NT) correct += joint_loss::row<false, true>(a, nullptr, 1.f, b, invB, l_cls, l_ord, l_unc, l_kan);
  }
  float r[5];
  joint_loss::reduce(a, invB, l_cls, l_ord, l_unc, l_kan, s_red, r);
  if (threadIdx.x == 0) {
    a.out[0] = r[0]; a.out[1] = r[1]; a.out[2] = r[2]; a.out[3] = r[3];
    a.out[4] = r[4];
  }
  if (!m.table) return;                          // uniform: a kernel argument
  correct = wave_sum_t(correct);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = correct;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* w = m.table + (size_t)m.row * RW;
    for (int k = 0; k < 5; ++k) w[ROVIT_TRAIN_ROW_LOSS + k] = __float_as_uint(r[k]);
    w[ROVIT_TRAIN_ROW_CORRECT] = (unsigned)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
    w[ROVIT_TRAIN_ROW_BATCH] = (unsigned)a.B;
    w[ROVIT_TRAIN_ROW_NONFINITE] = isfinite(r[4]) ? 0u : 1u;
  }
}

__global__ __launch_bounds__(NT) void train_final_kernel(const unsigned* __restrict__ table, int n_rows, long long* __restrict__ result) {
  __shared__ double s_d[4];
  __shared__ long long s_l[4];
  const int tid = threadIdx.x;
  long long samples = 0, correct = 0, bad = 0;
  for (int r = tid; r < n_rows; r += NT) {
    const unsigned* w = table + (size_t)r * RW;
    correct += w[ROVIT_TRAIN_ROW_CORRECT];
    samples += w[ROVIT_TRAIN_ROW_BATCH];
    bad += w[ROVIT_TRAIN_ROW_NONFINITE];
  }
  samples = block_sum_t(samples, s_l);
  correct = block_sum_t(correct, s_l);
  bad = block_sum_t(bad, s_l);
  if (tid == 0) {
    result[ROVIT_TRAIN_N_ROWS] = n_rows;
    result[ROVIT_TRAIN_SAMPLES] = samples;
    result[ROVIT_TRAIN_CORRECT] = correct;
    result[ROVIT_TRAIN_NONFINITE] = bad;
  }
  double* res = (double*)result;
  for (int k = 0; k < 5; ++k) {
    double s = 0.0;
    for (int r = tid; r < n_rows; r += NT) s += (double)__uint_as_float(table[(size_t)r * RW + ROVIT_TRAIN_ROW_LOSS + k]);
    s = block_sum_t(s, s_d);
    if (tid == 0) res[ROVIT_TRAIN_LOSS + k] = s;
  }
}

}  // namespace

extern "C" int rovit_joint_loss_mixed(const rovit_train_loss* p, rovit_stream_t stream) {
  const char* who = "joint_loss_mixed";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->cls_logits && p->class_targets_a && p->severity_targets && p->d_cls && p->losses_out, ROVIT_ERR_NULL,
                  "%s: logits, labels, the class gradient buffer or losses_out missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->batch > 0 && p->num_classes >= 2 && p->num_classes <= MAXC, ROVIT_ERR_SHAPE, "%s: batch %d (need >= 1), %d classes (need 2..%d)", who,
                  p->batch, p->num_classes, MAXC);
  ROVIT_CHECK_ARG((!p->ordinal_logits || p->d_ord) && (!p->mu || (p->log_var && p->d_mu && p->d_lv)) && (!p->kan_severity || p->d_kan),
                  ROVIT_ERR_NULL, "%s: gradient buffer missing for an active head", who);
  ROVIT_CHECK_ARG(!p->class_targets_b || (p->lam >= 0.f && p->lam <= 1.f), ROVIT_ERR_SHAPE, "%s: lam %g outside [0, 1]", who, (double)p->lam);
  ROVIT_CHECK_ARG(!p->table || (p->row >= 0 && p->capacity >= 1 && p->capacity <= ROVIT_TRAIN_MAX_ROWS && p->row < p->capacity), ROVIT_ERR_SHAPE,
                  "%s: row %d outside the epoch table (%d rows, at most %d)", who, p->row, p->capacity, ROVIT_TRAIN_MAX_ROWS);
  ROVIT_CHECK_ARG(rovit_aligned(p->cls_logits, 4) && rovit_aligned(p->ordinal_logits, 4) && rovit_aligned(p->mu, 4) && rovit_aligned(p->log_var, 4) &&
                      rovit_aligned(p->kan_severity, 4) && rovit_aligned(p->focal_alpha, 4) && rovit_aligned(p->class_targets_a, 8) &&
                      rovit_aligned(p->class_targets_b, 8) && rovit_aligned(p->severity_targets, p->severity_is_int64 ? 8 : 4),
                  ROVIT_ERR_ALIGN, "%s: an input pointer is not aligned to its element size", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->d_cls, 4) && rovit_aligned(p->d_ord, 4) && rovit_aligned(p->d_mu, 4) && rovit_aligned(p->d_lv, 4) && rovit_aligned(p->d_kan, 4) &&
                      rovit_aligned(p->losses_out, 4) && rovit_aligned(p->table, 4),
                  ROVIT_ERR_ALIGN, "%s: an output pointer is not 4-byte aligned", who);
  MixedArgs m{};
  m.l = LossArgs{p->cls_logits, p->ordinal_logits, p->mu, p->log_var, p->kan_severity, p->class_targets_a, p->severity_targets,
                 p->severity_is_int64 ? 1 : 0, p->focal_alpha, p->d_cls, p->d_ord, p->d_mu, p->d_lv, p->d_kan, p->losses_out, p->batch,
                 p->num_classes, p->lambda_ord, p->mu_unc, p->nu_kan, p->focal_gamma};
  m.cls_t_b = p->class_targets_b;
  m.lam = p->lam;
  m.table = (unsigned*)p->table;
  m.row = p->row;
  hipLaunchKernelGGL(joint_loss_mixed_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, m);
  ROVIT_CHECK_LAUNCH("joint_loss_mixed_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_train_finalize(const rovit_train_final* p, rovit_stream_t stream) {
  const char* who = "train_finalize";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->table && p->result, ROVIT_ERR_NULL, "%s: the epoch table or the result block is missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->n_rows >= 1 && p->n_rows <= p->capacity && p->capacity <= ROVIT_TRAIN_MAX_ROWS, ROVIT_ERR_SHAPE,
                  "%s: %d rows of a table of %d (1..capacity, at most %d)", who, p->n_rows, p->capacity, ROVIT_TRAIN_MAX_ROWS);
  ROVIT_CHECK_ARG(rovit_aligned(p->table, 4) && rovit_aligned(p->result, 8), ROVIT_ERR_ALIGN, "%s: the table or the result block is not aligned", who);
  hipLaunchKernelGGL(train_final_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const unsigned*)p->table, p->n_rows, (long long*)p->result);
  ROVIT_CHECK_LAUNCH("train_final_kernel");
  return ROVIT_OK;
}
