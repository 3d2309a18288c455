// Per-sample augmentation of a device-resident uint8 image store: gather by index, draw, resample, colour-transform, normalise and
// write the fp32 NCHW batch the backbone reads, in ONE launch (the specification of record is rovit_hip/augment.py's docstring;
// augment_reference there is the torch restatement the tests compare against).
//
// Reference call sites served: training/trainer.py:79-82 (`images, class_labels, severity_labels` of a train-loader batch, moved with
// .to(device)) and scripts/train.py:73-84 (create_dataloaders(..., augmented_transform=, original_transform=)).  The reference's
// data/transforms.py is NOT part of its checkout, so WHAT is augmented is this repository's own definition ("parity unpinned"): a
// RandomResizedCrop-style window, a rotation and flips as one affine map sampled bilinearly with clamped edges, then the DALI
// "ColorTwist" form of brightness / contrast / saturation / hue (one affine transform per pixel, one clamp), then ImageNet normalisation.
//
// Shape of the kernel.  One workgroup serves ONE sample: thread 0 draws (or reads) the 12-float parameter row and derives the affine map,
// the 3x3 colour matrix and its offset once, leaves them in LDS, and every lane reads them as wave-uniform values.  A lane owns 4
// consecutive output pixels of a row and stores one float4 per channel plane (the output is 80 % of the traffic).  The general path does
// 4 taps x 3 planes of byte loads per pixel from a source image that stays L2-resident across the workgroups sharing it; identity
// geometry on an equal-sized store (evaluation batches, the default flip + normalise config) reads one uchar4 per plane instead.
// A pixel's arithmetic does not depend on how the batch is split into launches or workgroups, and the draw is keyed by the image's index
// in the store: a given (image, seed, epoch) gives the same bits for every batch size, order and split.
//
// A store index outside [0, n_images) is never dereferenced: the sample's output (and its params_out row) is filled with NaN.
#include <math.h>

#include "common.h"
#include "philox.h"

namespace {

constexpr int AB_NT = 256;
constexpr int AB_ROW = 12;                       // floats per parameter row

struct AugArgs {
  const unsigned char* src; const long long* indices; const float* params; float* params_out; float* out;
  rovit_augment_config cfg;
  unsigned long long seed, epoch;
  int N, Hs, Ws, Ho, Wo, chunks, fast_ok;         // fast_ok: equal sizes and a 4-byte aligned store (host-checked)
};

enum { AB_GENERAL = 0, AB_FAST = 1, AB_BAD_INDEX = 2 };

// what thread 0 derives once per workgroup
struct AugSample {
  float m[9], off[3];                 // z = m . u8 + off (1/255, brightness and contrast folded in), clamped to [0, 1]
  float cx, cy;                       // source coordinate of the output centre (the -0.5 of the pixel-centre convention folded in)
  float mxx, mxy, myx, myy;           // d(sx, sy) / d(j, i)
  int mode, flip_h, flip_v;
  long long image;
};

// NTSC RGB -> YIQ rows 1, 2 and columns 1, 2 of the inverse (fp64 inverse of the 3x3 in the specification, rounded to fp32; its first
// column is (1, 1, 1), the luma row is untouched): A = I + TINV[:, 1:3] (s Rot(2 pi hue) - I) T[1:3, :]  -- exactly I at s = 1, hue = 0
__device__ __forceinline__ void colour_matrix(float sat, float hue, float A[9]) {
  const float T1[3] = {0.5959f, -0.2746f, -0.3213f}, T2[3] = {0.2115f, -0.5227f, 0.3112f};
  const float V1[3] = {0.9560502263958943f, -0.2720523436889242f, -1.1067043153243323f};
  const float V2[3] = {0.6207549413271234f, -0.6472057134551777f, 1.7044212836963109f};
  float sn, cs;
  sincosf(6.283185307179586f * hue, &sn, &cs);
  const float q00 = sat * cs - 1.f, q01 = -sat * sn, q10 = sat * sn, q11 = sat * cs - 1.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = V1[c] * q00 + V2[c] * q10, b = V1[c] * q01 + V2[c] * q11;      // row c of TINV[:, 1:3] Q
#pragma unroll
    for (int d = 0; d < 3; ++d) A[c * 3 + d] = (c == d ? 1.f : 0.f) + (a * T1[d] + b * T2[d]);
  }
}

__device__ void setup_sample(const AugArgs& a, int n, bool write_row, AugSample& s) {
  const long long image = a.indices[n];
  s.image = image;
  if (image < 0 || image >= a.N) {
    s.mode = AB_BAD_INDEX;
    if (write_row && a.params_out)
      for (int k = 0; k < AB_ROW; ++k) a.params_out[(size_t)n * AB_ROW + k] = __builtin_nanf("");
    return;
  }
  float row[AB_ROW];
  if (a.params) {
    for (int k = 0; k < AB_ROW; ++k) row[k] = a.params[(size_t)n * AB_ROW + k];
  } else {
    const rovit_augment_config& c = a.cfg;
    const unsigned e_lo = (unsigned)a.epoch, e_hi = (unsigned)(a.epoch >> 32);
    const U4 r0 = philox4x32_10(a.seed, (unsigned)image, 0u, e_lo, e_hi);
    const U4 r1 = philox4x32_10(a.seed, (unsigned)image, 1u, e_lo, e_hi);
    const U4 r2 = philox4x32_10(a.seed, (unsigned)image, 2u, e_lo, e_hi);
    row[0] = u01(r0.x) < c.p_hflip ? 1.f : 0.f;
    row[1] = u01(r0.y) < c.p_vflip ? 1.f : 0.f;
    row[2] = c.scale_lo + u01(r0.z) * (c.scale_hi - c.scale_lo);
    row[3] = c.log_ratio_lo + u01(r0.w) * (c.log_ratio_hi - c.log_ratio_lo);
    row[4] = u01(r1.x);
    row[5] = u01(r1.y);
    row[6] = (2.f * u01(r1.z) - 1.f) * c.theta_max;
    row[7] = 1.f + (2.f * u01(r1.w) - 1.f) * c.brightness;
    row[8] = 1.f + (2.f * u01(r2.x) - 1.f) * c.contrast;
    row[9] = 1.f + (2.f * u01(r2.y) - 1.f) * c.saturation;
    row[10] = (2.f * u01(r2.z) - 1.f) * c.hue;
    row[11] = 0.f;
  }
  if (write_row && a.params_out)
    for (int k = 0; k < AB_ROW; ++k) a.params_out[(size_t)n * AB_ROW + k] = row[k];

  // everything below is a function of the twelve floats alone: a drawn row and the same row passed back give the same bits
  s.flip_h = row[0] > 0.5f;
  s.flip_v = row[1] > 0.5f;
  const float area = row[2], log_ratio = row[3], theta = row[6];
  s.mode = (a.fast_ok && area == 1.f && log_ratio == 0.f && theta == 0.f) ? AB_FAST : AB_GENERAL;
  const float ratio = expf(log_ratio);
  const float Ws = (float)a.Ws, Hs = (float)a.Hs;
  const float w = fminf(Ws, Ws * sqrtf(area * ratio)), h = fminf(Hs, Hs * sqrtf(area / ratio));
  s.cx = row[4] * (Ws - w) + 0.5f * w - 0.5f;
  s.cy = row[5] * (Hs - h) + 0.5f * h - 0.5f;
  float sn, cs;
  sincosf(theta, &sn, &cs);
  const float px = (s.flip_h ? -w : w) / (float)a.Wo, py = (s.flip_v ? -h : h) / (float)a.Ho;   // source pixels per output pixel
  s.mxx = cs * px; s.mxy = -sn * py;
  s.myx = sn * px; s.myy = cs * py;
  float A[9];
  colour_matrix(row[9], row[10], A);
  const float bc = row[7] * row[8];
  for (int k = 0; k < 9; ++k) s.m[k] = A[k] * bc * (1.0f / 255.0f);
  const float off = row[7] * (0.5f - 0.5f * row[8]);          // brightness * (0.5 + contrast * (z - 0.5)) = bc z + off
  s.off[0] = s.off[1] = s.off[2] = off;
}

// colour transform, clamp, ImageNet normalisation of one pixel's three interpolated byte values
__device__ __forceinline__ void colour_norm(const AugSample& s, float r, float g, float b, float& o0, float& o1, float& o2) {
  float z0 = fmaf(s.m[0], r, fmaf(s.m[1], g, fmaf(s.m[2], b, s.off[0])));
  float z1 = fmaf(s.m[4], g, fmaf(s.m[3], r, fmaf(s.m[5], b, s.off[1])));
  float z2 = fmaf(s.m[8], b, fmaf(s.m[6], r, fmaf(s.m[7], g, s.off[2])));
  z0 = fminf(fmaxf(z0, 0.f), 1.f); z1 = fminf(fmaxf(z1, 0.f), 1.f); z2 = fminf(fmaxf(z2, 0.f), 1.f);
  o0 = fmaf(z0, (float)(1.0 / 0.229), -(float)(0.485 / 0.229));
  o1 = fmaf(z1, (float)(1.0 / 0.224), -(float)(0.456 / 0.224));
  o2 = fmaf(z2, (float)(1.0 / 0.225), -(float)(0.406 / 0.225));
}

__global__ __launch_bounds__(AB_NT) void augment_batch_kernel(const AugArgs a) {
  __shared__ AugSample sh;
  const int n = blockIdx.x / a.chunks, chunk = blockIdx.x - n * a.chunks;
  if (threadIdx.x == 0) setup_sample(a, n, chunk == 0, sh);
  __syncthreads();
  const AugSample& s = sh;
  const int W4 = a.Wo >> 2, items = a.Ho * W4;
  const size_t plane_o = (size_t)a.Ho * a.Wo, plane_s = (size_t)a.Hs * a.Ws;
  float* const out = a.out + (size_t)n * 3 * plane_o;
  const int mode = s.mode;

  if (mode == AB_BAD_INDEX) {
    const float q = __builtin_nanf("");
    for (int it = chunk * AB_NT + threadIdx.x; it < items; it += a.chunks * AB_NT)
#pragma unroll
      for (int c = 0; c < 3; ++c) reinterpret_cast<float4*>(out + c * plane_o)[it] = make_float4(q, q, q, q);
    return;
  }
  const unsigned char* const src = a.src + (size_t)s.image * 3 * plane_s;

  if (mode == AB_FAST) {
    // identity geometry: output pixel (i, j) is source pixel (i or Hs-1-i, j or Ws-1-j); one uchar4 per plane, reversed under flip_h
    for (int it = chunk * AB_NT + threadIdx.x; it < items; it += a.chunks * AB_NT) {
      const int i = it / W4, j4 = it - i * W4;
      const int si = s.flip_v ? a.Hs - 1 - i : i, sj4 = s.flip_h ? W4 - 1 - j4 : j4;
      uchar4 p[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[c] = reinterpret_cast<const uchar4*>(src + c * plane_s + (size_t)si * a.Ws)[sj4];
        if (s.flip_h) p[c] = make_uchar4(p[c].w, p[c].z, p[c].y, p[c].x);
      }
      float4 o[3];
      colour_norm(s, (float)p[0].x, (float)p[1].x, (float)p[2].x, o[0].x, o[1].x, o[2].x);
      colour_norm(s, (float)p[0].y, (float)p[1].y, (float)p[2].y, o[0].y, o[1].y, o[2].y);
      colour_norm(s, (float)p[0].z, (float)p[1].z, (float)p[2].z, o[0].z, o[1].z, o[2].z);
      colour_norm(s, (float)p[0].w, (float)p[1].w, (float)p[2].w, o[0].w, o[1].w, o[2].w);
#pragma unroll
      for (int c = 0; c < 3; ++c) reinterpret_cast<float4*>(out + c * plane_o)[it] = o[c];
    }
    return;
  }

  // general path: bilinear, clamped-edge taps.  A wave owns an 8-row x 32-pixel output tile (lane = 8 rows x 8 float4 columns), not 256
  // pixels of one row: under a rotation the tile's source footprint is ~24 cache lines per tap instead of one per lane pair, and every
  // row segment it stores is still 128 contiguous bytes.  The coordinate is built from the offset to the output centre (exact in fp32),
  // so its rounding error is a few ulp of the source side, not of an accumulated sum.
  const float jc = 0.5f * (float)(a.Wo - 1), ic = 0.5f * (float)(a.Ho - 1);
  const float xmax = (float)(a.Ws - 1), ymax = (float)(a.Hs - 1);
  const int tcols = (W4 + 7) >> 3, tiles = ((a.Ho + 7) >> 3) * tcols;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = chunk * (AB_NT / 64) + wave; t < tiles; t += a.chunks * (AB_NT / 64)) {
    const int tr = t / tcols;
    const int i = tr * 8 + (lane >> 3), j4 = (t - tr * tcols) * 8 + (lane & 7);
    if (i >= a.Ho || j4 >= W4) continue;
    const int it = i * W4 + j4;
    const float di = (float)i - ic;
    const float bx = fmaf(s.mxy, di, s.cx), by = fmaf(s.myy, di, s.cy);
    float o[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float dj = (float)(4 * j4 + e) - jc;
      const float sx = fminf(fmaxf(fmaf(s.mxx, dj, bx), 0.f), xmax);
      const float sy = fminf(fmaxf(fmaf(s.myx, dj, by), 0.f), ymax);
      const float fx0 = floorf(sx), fy0 = floorf(sy);
      const float fx = sx - fx0, fy = sy - fy0;
      const int x0 = (int)fx0, y0 = (int)fy0;
      const int x1 = min(x0 + 1, a.Ws - 1), y1 = min(y0 + 1, a.Hs - 1);
      const int r0 = y0 * a.Ws, r1 = y1 * a.Ws;
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned char* p = src + c * plane_s;
        const float t00 = (float)p[r0 + x0], t01 = (float)p[r0 + x1], t10 = (float)p[r1 + x0], t11 = (float)p[r1 + x1];
        const float top = fmaf(fx, t01 - t00, t00), bot = fmaf(fx, t11 - t10, t10);
        v[c] = fmaf(fy, bot - top, top);
      }
      colour_norm(s, v[0], v[1], v[2], o[0][e], o[1][e], o[2][e]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) reinterpret_cast<float4*>(out + c * plane_o)[it] = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
  }
}

bool in_unit(float p) { return p >= 0.f && p <= 1.f; }

}  // namespace

extern "C" int rovit_augment_batch(const unsigned char* src, int n_images, int src_h, int src_w, const long long* indices, int batch,
                                   const float* params, float* params_out, const rovit_augment_config* config,
                                   unsigned long long seed, unsigned long long epoch, float* out, int out_h, int out_w,
                                   rovit_stream_t stream) {
  ROVIT_CHECK_ARG(src && indices && out, ROVIT_ERR_NULL, "augment_batch: null pointer (src, indices, out)");
  ROVIT_CHECK_ARG(params || config, ROVIT_ERR_NULL, "augment_batch: no parameter rows and no config to draw them from");
  ROVIT_CHECK_ARG(n_images > 0 && src_h > 0 && src_w > 0, ROVIT_ERR_SHAPE, "augment_batch: empty store (%d images of %d x %d)", n_images,
                  src_h, src_w);
  ROVIT_CHECK_ARG(batch > 0 && out_h > 0 && out_w > 0, ROVIT_ERR_SHAPE, "augment_batch: empty output (%d x %d x %d)", batch, out_h, out_w);
  ROVIT_CHECK_ARG(out_w % 4 == 0, ROVIT_ERR_SHAPE, "augment_batch: output width %d is not a multiple of 4", out_w);
  ROVIT_CHECK_ARG(rovit_aligned16(out), ROVIT_ERR_ALIGN, "augment_batch: out must be 16-byte aligned");
  ROVIT_CHECK_ARG((size_t)src_h * src_w <= (size_t)1 << 28 && (size_t)out_h * out_w <= (size_t)1 << 28, ROVIT_ERR_SHAPE,
                  "augment_batch: image plane too large");
  const size_t items = (size_t)out_h * (out_w / 4);
  const size_t src_bytes = (size_t)n_images * 3 * src_h * src_w, out_bytes = (size_t)batch * 3 * out_h * out_w * sizeof(float);
  const uintptr_t s0 = (uintptr_t)src, o0 = (uintptr_t)out;
  ROVIT_CHECK_ARG(s0 + src_bytes <= o0 || o0 + out_bytes <= s0, ROVIT_ERR_SHAPE, "augment_batch: out aliases src");
  AugArgs a{};
  if (config) {
    const rovit_augment_config& c = *config;
    ROVIT_CHECK_ARG(in_unit(c.p_hflip) && in_unit(c.p_vflip), ROVIT_ERR_SHAPE, "augment_batch: flip probabilities (%g, %g) outside [0, 1]",
                    c.p_hflip, c.p_vflip);
    ROVIT_CHECK_ARG(c.scale_lo > 0.f && c.scale_lo <= c.scale_hi && c.scale_hi <= 1.f, ROVIT_ERR_SHAPE,
                    "augment_batch: scale range (%g, %g) must satisfy 0 < lo <= hi <= 1", c.scale_lo, c.scale_hi);
    ROVIT_CHECK_ARG(c.log_ratio_lo <= c.log_ratio_hi && isfinite(c.log_ratio_lo) && isfinite(c.log_ratio_hi), ROVIT_ERR_SHAPE,
                    "augment_batch: log aspect-ratio range (%g, %g) must be finite and ordered", c.log_ratio_lo, c.log_ratio_hi);
    ROVIT_CHECK_ARG(c.theta_max >= 0.f && c.brightness >= 0.f && c.contrast >= 0.f && c.saturation >= 0.f && c.hue >= 0.f &&
                        isfinite(c.theta_max + c.brightness + c.contrast + c.saturation + c.hue),
                    ROVIT_ERR_SHAPE, "augment_batch: rotation and jitter ranges must be finite and >= 0");
    a.cfg = c;
  }
  // workgroups per sample: enough of them to fill the device at small batches, at most ~8 passes of 256 lanes each at large ones
  const size_t max_chunks = (items + AB_NT - 1) / AB_NT;
  size_t chunks = (size_t)(2048 + batch - 1) / batch;
  const size_t by_work = (items + 8 * AB_NT - 1) / (8 * AB_NT);
  if (chunks < by_work) chunks = by_work;
  if (chunks > max_chunks) chunks = max_chunks;
  ROVIT_CHECK_ARG((size_t)batch * chunks < (size_t)1 << 31, ROVIT_ERR_SHAPE, "augment_batch: batch %d too large for one launch", batch);
  a.src = src; a.indices = indices; a.params = params; a.params_out = params_out; a.out = out;
  a.seed = seed; a.epoch = epoch;
  a.N = n_images; a.Hs = src_h; a.Ws = src_w; a.Ho = out_h; a.Wo = out_w; a.chunks = (int)chunks;
  a.fast_ok = src_h == out_h && src_w == out_w && ((uintptr_t)src & 3u) == 0;      // out_w % 4 == 0, so every row stays 4-byte aligned
  hipLaunchKernelGGL(augment_batch_kernel, dim3((unsigned)((size_t)batch * chunks)), dim3(AB_NT), 0, (hipStream_t)stream, a);
  ROVIT_CHECK_LAUNCH("augment_batch_kernel");
  return ROVIT_OK;
}
