// Fused joint multi-task loss, forward + gradient in one launch.
//
// Reference being restated: training/losses.py JointLoss.forward :139-181; the formulas are stated once, in joint_loss_row.h.
// One workgroup walks the batch (B is a few hundred rows, 4+3+1+1+1 values per row); the per-row gradients of the
// TOTAL loss w.r.t. every head output are written in the same pass, so backward is a single scale by the upstream
// gradient instead of ~25 elementwise/reduction launches.
#include "common.h"
#include "joint_loss_row.h"      // the per-row arithmetic and the block reduction, shared with train_epoch.hip

namespace {

using joint_loss::LossArgs;
using joint_loss::MAXC;

__global__ __launch_bounds__(256) void joint_loss_kernel(const LossArgs a) {
  __shared__ float s_red[4];
  const float invB = 1.f / a.B;
  float l_cls = 0.f, l_ord = 0.f, l_unc = 0.f, l_kan = 0.f;
  for (int b = threadIdx.x; b < a.B; b += 256) joint_loss::row<false, false>(a, nullptr, 1.f, b, invB, l_cls, l_ord, l_unc, l_kan);
  float r[5];
  joint_loss::reduce(a, invB, l_cls, l_ord, l_unc, l_kan, s_red, r);
  if (threadIdx.x == 0) {
    a.out[0] = r[0]; a.out[1] = r[1]; a.out[2] = r[2]; a.out[3] = r[3];
    a.out[4] = r[4];
  }
}

// g[i] *= *scale for up to 5 small buffers (the backward of the loss: chain with the upstream gradient)
struct ScaleArgs { float* p[5]; int n[5]; const float* scale; };
__global__ __launch_bounds__(256) void scale_buffers_kernel(const ScaleArgs a) {
  const float s = *a.scale;
  for (int k = 0; k < 5; ++k)
    if (a.p[k])
      for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n[k]; i += gridDim.x * 256) a.p[k][i] *= s;
}

}  // namespace

// Inactive heads: pass NULL for (ord, d_ord) / (mu, lv, d_mu, d_lv) / (kan, d_kan) -- that is the curriculum gate.
// d_* receive d(total)/d(output) for an upstream gradient of 1.  losses_out: [cls, ord, unc, kan, total].
extern "C" int rovit_joint_loss(const float* cls_logits, const float* ordinal_logits, const float* mu, const float* log_var,
                                const float* kan_severity, const long long* class_targets, const void* severity_targets,
                                int severity_is_int64, const float* focal_alpha, float* d_cls, float* d_ord, float* d_mu, float* d_lv, float* d_kan,
                                float* losses_out, int batch, int num_classes, float lambda_ord, float mu_unc, float nu_kan,
                                float focal_gamma, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(cls_logits && class_targets && severity_targets && d_cls && losses_out, ROVIT_ERR_NULL, "joint_loss: null pointer");
  ROVIT_CHECK_ARG(batch > 0 && num_classes >= 2 && num_classes <= MAXC, ROVIT_ERR_SHAPE, "joint_loss: bad batch/classes");
  ROVIT_CHECK_ARG((!ordinal_logits || d_ord) && (!mu || (log_var && d_mu && d_lv)) && (!kan_severity || d_kan), ROVIT_ERR_NULL,
                  "joint_loss: gradient buffer missing for an active head");
  LossArgs a{cls_logits, ordinal_logits, mu, log_var, kan_severity, class_targets, severity_targets, severity_is_int64 ? 1 : 0, focal_alpha,
             d_cls, d_ord, d_mu, d_lv, d_kan, losses_out, batch, num_classes, lambda_ord, mu_unc, nu_kan, focal_gamma};
  hipLaunchKernelGGL(joint_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  ROVIT_CHECK_LAUNCH("joint_loss_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_scale_buffers(float* const* bufs, const int* counts, int n, const float* scale, rovit_stream_t stream) {
  ROVIT_CHECK_ARG(bufs && counts && scale && n >= 1 && n <= 5, ROVIT_ERR_SHAPE, "scale_buffers: 1..5 buffers");
  ScaleArgs a{};
  int mx = 0;
  for (int i = 0; i < n; ++i) { a.p[i] = bufs[i]; a.n[i] = counts[i]; mx = counts[i] > mx ? counts[i] : mx; }
  a.scale = scale;
  hipLaunchKernelGGL(scale_buffers_kernel, dim3((mx + 255) / 256 > 0 ? (mx + 255) / 256 : 1), dim3(256), 0, (hipStream_t)stream, a);
  ROVIT_CHECK_LAUNCH("scale_buffers_kernel");
  return ROVIT_OK;
}
