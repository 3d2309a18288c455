// Projected-gradient attack steps on normalised images (include/rovit_hip.h "Adversarial perturbations"; the specification of record
// is rovit_hip/attack.py: step_reference / init_reference).  Memory-bound elementwise kernels over a grid of (image, channel, slab of
// AT_SLAB pixels): 16-byte loads and stores when H W is a multiple of 4 and every pointer is 16-byte aligned, one element per access
// otherwise.  The L-infinity step and start are one launch and fp32 with one rounding per operation, so that numpy restates them to
// the bit; the L2 forms need two image-wide norms, which are fp64 sums in a fixed order (per-slab partials in scratch, then every
// workgroup of the image adds the image's partials in index order): no atomic, nothing that depends on the grid.
#include "common.h"
#include "philox.h"
#include <cmath>

constexpr int AT_NT = 256;              // threads of a workgroup (four waves)
constexpr int AT_SLAB = 4 * AT_NT;      // pixels of one channel plane per workgroup

struct AttackConst { float inv_s[3], s[3], lo[3], hi[3]; };
struct AttackArgs {
  const float* x; const float* g; float* delta; float* x_adv; float* best_delta;
  const unsigned char* copy_mask; const float* eps; const float* alpha; const long long* ids;
  double* scratch;                      // L2: two sections of B * 3 * slabs partial sums
  AttackConst k;
  int n, slabs, init;                   // pixels per plane; slabs per plane; the L2 middle launch serves rovit_attack_init
  unsigned long long seed; unsigned restart;
};

// lo when v < lo, hi when v > hi, else v itself: a zero keeps its sign and a NaN passes through, which fminf / fmaxf leave open
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Every fp32 operation of the L-infinity forms is rounded once and on its own: the functions below switch contraction off (hipcc's
// default would fuse a * b + c, and __fadd_rn / __fmul_rn are plain operators to it, so they would not stop that).
// ball, box, ball again, box again: |dn| <= r and lo <= xa <= hi hold exactly; xa - x may differ from dn by the rounding of x + dn
__device__ __forceinline__ void project_linf(float x, float d1, float r, float lo, float hi, float& dn, float& xa) {
#pragma clang fp contract(off)
  const float d2 = clampf(d1, -r, r);
  const float y = clampf(x + d2, lo, hi);
  dn = clampf(y - x, -r, r);
  xa = clampf(x + dn, lo, hi);
}

__device__ __forceinline__ void step_linf(float x, float g, float d, float a, float r, float lo, float hi, float& dn, float& xa) {
#pragma clang fp contract(off)
  const float sg = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);          // 0 for +-0 and NaN
  const float move = sg * a;                                        // exact
  project_linf(x, d + move, r, lo, hi, dn, xa);
}

__device__ __forceinline__ void start_linf(float x, unsigned w, float r, float lo, float hi, float& dn, float& xa) {
#pragma clang fp contract(off)
  const float t = 2.f * u01(w) - 1.f;                               // exact: a multiple of 2^-23 in [-1, 1)
  project_linf(x, t * r, r, lo, hi, dn, xa);
}

__device__ __forceinline__ unsigned word_of(const U4& w, int j) { return j == 0 ? w.x : j == 1 ? w.y : j == 2 ? w.z : w.w; }

// Box-Muller in fp64: words (x, y) give the normals of elements 4k (cosine) and 4k + 1 (sine), words (z, w) those of 4k + 2 and 4k + 3
__device__ __forceinline__ double normal_of(const U4& w, int j) {
  const unsigned wa = j < 2 ? w.x : w.z, wb = j < 2 ? w.y : w.w;
  const double rad = sqrt(-2.0 * log((double)((wa >> 8) + 1u) * (1.0 / 16777216.0)));
  const double ang = 6.283185307179586476925 * ((double)(wb >> 8) * (1.0 / 16777216.0));
  return rad * ((j & 1) ? sin(ang) : cos(ang));
}

struct Where { int b, c; size_t base; int i0; size_t part; };
__device__ __forceinline__ Where where(const AttackArgs& a) {
  const unsigned blk = blockIdx.x;
  const int slab = (int)(blk % (unsigned)a.slabs), c = (int)((blk / (unsigned)a.slabs) % 3u), b = (int)(blk / (3u * (unsigned)a.slabs));
  return Where{b, c, ((size_t)b * 3 + c) * (size_t)a.n, slab * AT_SLAB, (size_t)b * 3 * a.slabs + (size_t)c * a.slabs + slab};
}

// Walks the workgroup's slab: f(offset in the tensor, lane of the element in its group of four) per element.  VEC: a thread owns four
// consecutive elements (the caller moves them with one 16-byte access); otherwise elements i0 + k * AT_NT + tid.
template <bool VEC, typename F>
__device__ __forceinline__ void for_slab(const AttackArgs& a, const Where& w, F f) {
  if (VEC) {
    const int i = w.i0 + (int)threadIdx.x * 4;
    if (i < a.n) f(w.base + i, i);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = w.i0 + k * AT_NT + (int)threadIdx.x;
      if (i < a.n) f(w.base + i, i);
    }
  }
}

template <bool VEC> struct Pack;
template <> struct Pack<true> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) { const f32x4 t = *reinterpret_cast<const f32x4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  __device__ __forceinline__ void store(float* p) const { f32x4 t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3]; *reinterpret_cast<f32x4*>(p) = t; }
  static constexpr int N = 4;
};
template <> struct Pack<false> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
  static constexpr int N = 1;
};

// ---- L-infinity: one launch ---------------------------------------------------------------------------------------------------------
template <bool VEC, bool INIT>
__global__ __launch_bounds__(AT_NT) void attack_linf_kernel(AttackArgs a) {
  const Where w = where(a);
  const float inv_s = a.k.inv_s[w.c], lo = a.k.lo[w.c], hi = a.k.hi[w.c];
  const float r = a.eps[w.b] * inv_s;
  const float al = INIT ? 0.f : a.alpha[w.b] * inv_s;
  const bool copy = !INIT && a.copy_mask && a.copy_mask[w.b] != 0;
  const unsigned id = INIT ? (unsigned)a.ids[w.b] : 0u;
  const size_t plane = (size_t)w.c * (size_t)a.n;
  for_slab<VEC>(a, w, [&](size_t off, int i) {
    Pack<VEC> x, d, g, xa;
    x.load(a.x + off);
    if (INIT) {
      const size_t e = plane + (size_t)i;                            // the element's index in its image
      const U4 words = philox4x32_10(a.seed, (unsigned)(e >> 2), id, ROVIT_ATTACK_STREAM, a.restart);
#pragma unroll
      for (int j = 0; j < Pack<VEC>::N; ++j) start_linf(x.v[j], word_of(words, VEC ? j : (int)(e & 3)), r, lo, hi, d.v[j], xa.v[j]);
    } else {
      d.load(a.delta + off);
      g.load(a.g + off);
      if (copy) d.store(a.best_delta + off);
#pragma unroll
      for (int j = 0; j < Pack<VEC>::N; ++j) step_linf(x.v[j], g.v[j], d.v[j], al, r, lo, hi, d.v[j], xa.v[j]);
    }
    d.store(a.delta + off);
    xa.store(a.x_adv + off);
  });
}

// ---- L2: three launches ---------------------------------------------------------------------------------------------------------------
// the image's partials, added in index order by every thread alike (a uniform loop: the same value in every lane and workgroup)
__device__ __forceinline__ double image_sum(const double* part, int b, int count) {
  const double* p = part + (size_t)b * count;
  double t = 0.0;
  for (int k = 0; k < count; ++k) t += p[k];
  return t;
}

// first launch.  Step: the partial sums of (g inv_s)^2, a non-finite g counting as 0.  Start: the fp64 normals, rounded once into delta,
// and the partial sums of their squares (of the rounded values, which the next launch reads).
template <bool VEC, bool INIT>
__global__ __launch_bounds__(AT_NT) void attack_l2_norm_kernel(AttackArgs a) {
  __shared__ double lds[AT_NT / 64];
  const Where w = where(a);
  const double inv_s = (double)a.k.inv_s[w.c];
  const unsigned id = INIT ? (unsigned)a.ids[w.b] : 0u;
  const size_t plane = (size_t)w.c * (size_t)a.n;
  double acc = 0.0;
  for_slab<VEC>(a, w, [&](size_t off, int i) {
    Pack<VEC> v;
    if (INIT) {
      const size_t e = plane + (size_t)i;
      const U4 words = philox4x32_10(a.seed, (unsigned)(e >> 2), id, ROVIT_ATTACK_STREAM, a.restart);
#pragma unroll
      for (int j = 0; j < Pack<VEC>::N; ++j) {
        v.v[j] = (float)normal_of(words, VEC ? j : (int)(e & 3));
        acc += (double)v.v[j] * (double)v.v[j];
      }
      v.store(a.delta + off);
    } else {
      v.load(a.g + off);
#pragma unroll
      for (int j = 0; j < Pack<VEC>::N; ++j) {
        const double gh = isfinite(v.v[j]) ? (double)v.v[j] * inv_s : 0.0;
        acc += gh * gh;
      }
    }
  });
  const double total = block_sum_t<AT_NT / 64>(acc, lds);
  if (threadIdx.x == 0) a.scratch[w.part] = total;
}

// second launch: the move, made in pixel units and added in normalised units, the box in delta space (delta in [lo - x, hi - x]: the move is never
// added to x before it is bounded, so no rounding of x enters it), delta rounded once; partial sums of (delta s)^2 into section 1.
template <bool VEC>
__global__ __launch_bounds__(AT_NT) void attack_l2_move_kernel(AttackArgs a) {
  __shared__ double lds[AT_NT / 64];
  const Where w = where(a);
  const int count = 3 * a.slabs;
  const double inv_s = (double)a.k.inv_s[w.c], s = (double)a.k.s[w.c], lo = (double)a.k.lo[w.c], hi = (double)a.k.hi[w.c];
  const double g2 = image_sum(a.scratch, w.b, count);
  const double len = (double)(a.init ? a.eps[w.b] : a.alpha[w.b]);
  const double t = g2 > 0.0 ? len / sqrt(g2) : 0.0;                 // a zero norm: no move
  const bool copy = !a.init && a.copy_mask && a.copy_mask[w.b] != 0;
  const bool init = a.init != 0;
  double acc = 0.0;
  for_slab<VEC>(a, w, [&](size_t off, int) {
    Pack<VEC> x, d, g;
    x.load(a.x + off);
    d.load(a.delta + off);
    if (!init) g.load(a.g + off);
    if (copy) d.store(a.best_delta + off);
#pragma unroll
    for (int j = 0; j < Pack<VEC>::N; ++j) {
      const double gh = init ? (double)d.v[j] : (isfinite(g.v[j]) ? (double)g.v[j] * inv_s : 0.0);
      const double d1 = (init ? 0.0 : (double)d.v[j]) + gh * t * inv_s;       // delta itself is not scaled: no move, no change
      const float db = (float)clampd(d1, lo - (double)x.v[j], hi - (double)x.v[j]);
      const double ub = (double)db * s;
      acc += ub * ub;
      d.v[j] = db;
    }
    d.store(a.delta + off);
  });
  const double total = block_sum_t<AT_NT / 64>(acc, lds);
  if (threadIdx.x == 0) a.scratch[(size_t)gridDim.x + w.part] = total;
}

// third launch: shrink to the ball (one factor per image, fp64, the product rounded once), then x_adv inside the box exactly
template <bool VEC>
__global__ __launch_bounds__(AT_NT) void attack_l2_shrink_kernel(AttackArgs a) {
  const Where w = where(a);
  const float lo = a.k.lo[w.c], hi = a.k.hi[w.c];
  const double un = sqrt(image_sum(a.scratch + (size_t)gridDim.x, w.b, 3 * a.slabs));
  const double eps = (double)a.eps[w.b];
  const double f = un > eps ? eps / un : 1.0;
  for_slab<VEC>(a, w, [&](size_t off, int) {
    Pack<VEC> x, d, xa;
    x.load(a.x + off);
    d.load(a.delta + off);
#pragma unroll
    for (int j = 0; j < Pack<VEC>::N; ++j) {
      d.v[j] = (float)((double)d.v[j] * f);
      xa.v[j] = clampf(x.v[j] + d.v[j], lo, hi);
    }
    d.store(a.delta + off);
    xa.store(a.x_adv + off);
  });
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static int attack_slabs(long long n) { return (int)((n + AT_SLAB - 1) / AT_SLAB); }

extern "C" size_t rovit_attack_scratch_doubles(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || (long long)H * W > (1ll << 28)) return 0;
  const unsigned long long words = 2ull * (unsigned long long)B * 3ull * (unsigned long long)attack_slabs((long long)H * W);
  return words < (1ull << 31) ? (size_t)words : 0;
}

static bool overlap(const void* p, const void* q, size_t bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && a < b + bytes && b < a + bytes;
}

// the checks every entry point shares; fills the constants and the shape
static int attack_common(const char* what, AttackArgs& a, const float* inv_s, const float* s, const float* lo, const float* hi, int B, int H,
                         int W, bool& vec) {
  ROVIT_CHECK_ARG(a.x && a.delta && a.x_adv && a.eps && inv_s && lo && hi, ROVIT_ERR_NULL,
                  "%s: null pointer (x, delta, x_adv, eps, inv_s, lo, hi)", what);
  ROVIT_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, ROVIT_ERR_SHAPE, "%s: B = %d images of %d x %d (every one must be >= 1)", what, B, H, W);
  const long long n = (long long)H * W;
  ROVIT_CHECK_ARG(n <= (1ll << 28), ROVIT_ERR_SHAPE, "%s: image plane too large", what);
  const int slabs = attack_slabs(n);
  ROVIT_CHECK_ARG((unsigned long long)B * 3ull * (unsigned long long)slabs < (1ull << 30), ROVIT_ERR_SHAPE, "%s: batch %d too large for one launch",
                  what, B);
  for (int c = 0; c < 3; ++c) {
    ROVIT_CHECK_ARG(std::isfinite(inv_s[c]) && inv_s[c] > 0.f, ROVIT_ERR_SHAPE, "%s: inv_s[%d] = %g must be finite and positive", what, c, inv_s[c]);
    ROVIT_CHECK_ARG(!s || (std::isfinite(s[c]) && s[c] > 0.f), ROVIT_ERR_SHAPE, "%s: s[%d] = %g must be finite and positive", what, c, s ? s[c] : 0.f);
    ROVIT_CHECK_ARG((std::isfinite(lo[c]) || lo[c] == -INFINITY) && (std::isfinite(hi[c]) || hi[c] == INFINITY) && lo[c] <= hi[c], ROVIT_ERR_SHAPE,
                    "%s: box [%g, %g] of channel %d (finite, or -inf / +inf for no box; lo <= hi)", what, lo[c], hi[c], c);
    a.k.inv_s[c] = inv_s[c]; a.k.s[c] = s ? s[c] : 0.f; a.k.lo[c] = lo[c]; a.k.hi[c] = hi[c];
  }
  const size_t bytes = (size_t)B * 3 * (size_t)n * sizeof(float);
  ROVIT_CHECK_ARG(!overlap(a.x, a.delta, bytes) && !overlap(a.x, a.x_adv, bytes) && !overlap(a.delta, a.x_adv, bytes) &&
                      !overlap(a.g, a.delta, bytes) && !overlap(a.g, a.x_adv, bytes) && !overlap(a.best_delta, a.delta, bytes) &&
                      !overlap(a.best_delta, a.x_adv, bytes) && !overlap(a.best_delta, a.x, bytes) && !overlap(a.best_delta, a.g, bytes),
                  ROVIT_ERR_SHAPE, "%s: x, g, delta, x_adv and best_delta must not overlap", what);
  ROVIT_CHECK_ARG(rovit_aligned(a.x, 4) && rovit_aligned(a.g, 4) && rovit_aligned(a.delta, 4) && rovit_aligned(a.x_adv, 4) &&
                      rovit_aligned(a.best_delta, 4) && rovit_aligned(a.scratch, 8),
                  ROVIT_ERR_ALIGN, "%s: fp32 tensors must be 4-byte aligned, scratch 8-byte aligned", what);
  a.n = (int)n;
  a.slabs = slabs;
  vec = n % 4 == 0 && rovit_aligned16(a.x) && rovit_aligned16(a.g) && rovit_aligned16(a.delta) && rovit_aligned16(a.x_adv) &&
        rovit_aligned16(a.best_delta);
  return ROVIT_OK;
}

static int step_pointers(const char* what, const AttackArgs& a) {
  ROVIT_CHECK_ARG(a.g && a.alpha, ROVIT_ERR_NULL, "%s: null pointer (g, alpha)", what);
  ROVIT_CHECK_ARG((a.best_delta != nullptr) == (a.copy_mask != nullptr), ROVIT_ERR_NULL, "%s: best_delta and copy_mask go together", what);
  return ROVIT_OK;
}

#define AT_LAUNCH(kernel)                                                                           \
  do {                                                                                              \
    if (vec) hipLaunchKernelGGL((kernel<true>), grid, dim3(AT_NT), 0, (hipStream_t)stream, a);      \
    else hipLaunchKernelGGL((kernel<false>), grid, dim3(AT_NT), 0, (hipStream_t)stream, a);         \
    ROVIT_CHECK_LAUNCH(#kernel);                                                                    \
  } while (0)
#define AT_LAUNCH2(kernel, flag)                                                                        \
  do {                                                                                                  \
    if (vec) hipLaunchKernelGGL((kernel<true, flag>), grid, dim3(AT_NT), 0, (hipStream_t)stream, a);    \
    else hipLaunchKernelGGL((kernel<false, flag>), grid, dim3(AT_NT), 0, (hipStream_t)stream, a);       \
    ROVIT_CHECK_LAUNCH(#kernel);                                                                        \
  } while (0)

extern "C" int rovit_attack_step_linf(const float* x, const float* g, float* delta, float* x_adv, float* best_delta,
                                      const unsigned char* copy_mask, const float* eps, const float* alpha, const float* inv_s, const float* lo,
                                      const float* hi, int B, int H, int W, rovit_stream_t stream) {
  AttackArgs a = {};
  a.x = x; a.g = g; a.delta = delta; a.x_adv = x_adv; a.best_delta = best_delta; a.copy_mask = copy_mask; a.eps = eps; a.alpha = alpha;
  bool vec = false;
  int rc = step_pointers("attack_step_linf", a);
  if (rc != ROVIT_OK) return rc;
  rc = attack_common("attack_step_linf", a, inv_s, nullptr, lo, hi, B, H, W, vec);
  if (rc != ROVIT_OK) return rc;
  const dim3 grid((unsigned)B * 3u * (unsigned)a.slabs);
  AT_LAUNCH2(attack_linf_kernel, false);
  return ROVIT_OK;
}

extern "C" int rovit_attack_step_l2(const float* x, const float* g, float* delta, float* x_adv, float* best_delta, const unsigned char* copy_mask,
                                    const float* eps, const float* alpha, const float* inv_s, const float* s, const float* lo, const float* hi,
                                    double* scratch, int B, int H, int W, rovit_stream_t stream) {
  AttackArgs a = {};
  a.x = x; a.g = g; a.delta = delta; a.x_adv = x_adv; a.best_delta = best_delta; a.copy_mask = copy_mask; a.eps = eps; a.alpha = alpha;
  a.scratch = scratch;
  bool vec = false;
  int rc = step_pointers("attack_step_l2", a);
  if (rc != ROVIT_OK) return rc;
  ROVIT_CHECK_ARG(s && scratch, ROVIT_ERR_NULL, "attack_step_l2: null pointer (s, scratch)");
  rc = attack_common("attack_step_l2", a, inv_s, s, lo, hi, B, H, W, vec);
  if (rc != ROVIT_OK) return rc;
  const dim3 grid((unsigned)B * 3u * (unsigned)a.slabs);
  AT_LAUNCH2(attack_l2_norm_kernel, false);
  AT_LAUNCH(attack_l2_move_kernel);
  AT_LAUNCH(attack_l2_shrink_kernel);
  return ROVIT_OK;
}

extern "C" int rovit_attack_init(const float* x, float* delta, float* x_adv, const long long* ids, const float* eps, int norm,
                                 unsigned long long seed, unsigned restart, const float* inv_s, const float* s, const float* lo, const float* hi,
                                 double* scratch, int B, int H, int W, rovit_stream_t stream) {
  AttackArgs a = {};
  a.x = x; a.delta = delta; a.x_adv = x_adv; a.ids = ids; a.eps = eps; a.scratch = scratch; a.seed = seed; a.restart = restart; a.init = 1;
  bool vec = false;
  ROVIT_CHECK_ARG(norm == ROVIT_ATTACK_LINF || norm == ROVIT_ATTACK_L2, ROVIT_ERR_SHAPE, "attack_init: norm %d (ROVIT_ATTACK_LINF or _L2)", norm);
  ROVIT_CHECK_ARG(ids, ROVIT_ERR_NULL, "attack_init: null pointer (ids)");
  ROVIT_CHECK_ARG(norm == ROVIT_ATTACK_LINF || (s && scratch), ROVIT_ERR_NULL, "attack_init: the L2 start needs s and scratch");
  const int rc = attack_common("attack_init", a, inv_s, norm == ROVIT_ATTACK_L2 ? s : nullptr, lo, hi, B, H, W, vec);
  if (rc != ROVIT_OK) return rc;
  const dim3 grid((unsigned)B * 3u * (unsigned)a.slabs);
  if (norm == ROVIT_ATTACK_LINF) {
    AT_LAUNCH2(attack_linf_kernel, true);
    return ROVIT_OK;
  }
  AT_LAUNCH2(attack_l2_norm_kernel, true);
  AT_LAUNCH(attack_l2_move_kernel);
  AT_LAUNCH(attack_l2_shrink_kernel);
  return ROVIT_OK;
}
