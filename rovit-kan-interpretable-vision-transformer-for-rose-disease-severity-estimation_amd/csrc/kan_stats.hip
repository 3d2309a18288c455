// Per-edge activation statistics of one KAN layer over a data set (rovit_kan_edge_stats) and every edge's curve at once
// (rovit_kan_curves).
//
// Reference being extended: models/kan.py:70-95 (the edge functions) and :97-114 (plot_activation, one edge per call);
// explainability/kan_viz.py plots a handful of such curves and says nothing about where the data falls on them.
//
// For the layer's N input rows a (N, in):   s_ij(x) = sum_k spline_w[i,j,k] B_k(tanh x)    phi_ij(x) = lin_w[j,i] x + s_ij(x)
//                                           z_nj = lin_b[j] + sum_i phi_ij(a_ni)
// result section (8-byte words, E = in * out; include/rovit_hip.h):
//   double [q E + i out + j]  q = 0..4: sum phi, sum phi^2, sum |phi|, sum |s|, |lin_w[j,i]| sum |a_i|
//   double [5E + j], [5E + out + j]: sum z, sum z^2     double [5E + 2 out + i]: sum |a_i|
//   int64 [.. + i nk + t]: rows with tanh(a_i) in knot interval t      int64 non-finite inputs, n
//
// Two evaluation kernels and one fold, all on the caller's stream behind one memset of the section:
//   kan_edge_kernel  a workgroup owns TI inputs x 64 outputs and a fixed range of 64-row chunks.  Per chunk the (row, input) pairs get
//                    tanhf and kan_basis ONCE, cooperatively, into LDS (x, interval, the four live basis values); thread (row group, output)
//                    reads them as a broadcast, gathers its four live coefficients from the LDS weight tile (transposed to (input, basis,
//                    output): lanes are consecutive outputs, so consecutive banks) and updates 4 fp32 sums per edge, folded into fp64 after
//                    every chunk (at most 16 rows per thread: the error does not grow with N).  No edge value is ever stored.
//   kan_pre_kernel   a workgroup owns 64 rows x 64 outputs and walks ALL inputs, z in registers: sum z, sum z^2; its staging phase also owns
//                    the interval counts (integer atomics), the non-finite count and sum |a_i|.
//   kan_fold_kernel  adds the per-range / per-chunk fp64 partials in index order.
// Every partition (TI, the row ranges, the chunks) is a function of N and the layer shape only and every floating sum has a fixed order,
// so the section is bit-identical from run to run; integers are order-free.
#include "kan_device.h"

namespace {

constexpr int NT = 256;                 // threads per workgroup
constexpr int SR = 64;                  // rows per chunk
constexpr int OT = 64;                  // outputs per workgroup
constexpr int RPT = 16;                 // rows per thread and chunk at most (SR / (NT / OT))
constexpr int MAX_SPLITS = 64;          // row ranges of the edge kernel at most
constexpr int LDS_BUDGET = 48 * 1024;

struct Geometry {
  int ow;        // lanes per row group: smallest power of two >= min(out, 64)
  int ti;        // inputs per tile: 4, 2 or 1
  int tiles, otiles, chunks, splits, chunks_per_split;
  size_t lds;
};

static inline size_t lds_bytes(int ti, int nb, int ow) {
  return (size_t)ti * nb * ow * 4 + (size_t)SR * ti * 32 + NT * 8 + (size_t)ti * KAN_MAX_KNOTS * 4 + KAN_MAX_KNOTS * 4;
}

static Geometry geometry(int n, int in_f, int out_f, int nk) {
  Geometry g;
  const int nb = nk - 4, o = out_f < OT ? out_f : OT;
  g.ow = 1;
  while (g.ow < o) g.ow <<= 1;
  g.ti = 4;
  while (g.ti > 1 && lds_bytes(g.ti, nb, g.ow) > (size_t)LDS_BUDGET) g.ti >>= 1;
  g.lds = lds_bytes(g.ti, nb, g.ow);
  g.tiles = (in_f + g.ti - 1) / g.ti;
  g.otiles = (out_f + OT - 1) / OT;
  g.chunks = (n + SR - 1) / SR;
  long want = (2048 + (long)g.tiles * g.otiles - 1) / ((long)g.tiles * g.otiles);       // about eight workgroups per CU
  int s = (int)(want < 1 ? 1 : (want > MAX_SPLITS ? MAX_SPLITS : want));
  s = s > g.chunks ? g.chunks : s;
  g.chunks_per_split = (g.chunks + s - 1) / s;
  g.splits = (g.chunks + g.chunks_per_split - 1) / g.chunks_per_split;
  return g;
}

struct Lds {
  float* w;            // (ti, nb, ow) coefficients of the tile
  float4* stage;       // (SR, ti, 2): {x, interval bits, v0, v1}, {v2, v3, -, -}
  double* red;         // NT
  unsigned* occ;       // (ti, nk) interval counts of the tile
  float* knots;        // nk
};

__device__ __forceinline__ Lds carve(unsigned char* base, int ti, int nb, int ow) {
  Lds l;
  l.stage = reinterpret_cast<float4*>(base);                      base += (size_t)SR * ti * 32;
  l.red = reinterpret_cast<double*>(base);                        base += NT * 8;
  l.w = reinterpret_cast<float*>(base);                           base += (size_t)ti * nb * ow * 4;
  l.occ = reinterpret_cast<unsigned*>(base);                      base += (size_t)ti * KAN_MAX_KNOTS * 4;
  l.knots = reinterpret_cast<float*>(base);
  return l;
}

// spline_w (in, out, nb) rows [i0, i0 + TI) x outputs [j0, j0 + ow) -> LDS (TI, nb, ow); out-of-range entries are zero
template <int TI>
__device__ __forceinline__ void load_weight_tile(const rovit_kan_stats& a, float* w, int i0, int j0, int nb, int ow) {
  const int total = TI * nb * ow;
  for (int idx = threadIdx.x; idx < total; idx += NT) {
    const int jj = idx % ow, k = (idx / ow) % nb, il = idx / (ow * nb);
    const int i = i0 + il, j = j0 + jj;
    w[idx] = (i < a.in_f && j < a.out_f) ? a.spline_w[((size_t)i * a.out_f + j) * nb + k] : 0.f;
  }
}

// tanhf and the basis once per (row, input) of the chunk; COUNT: the interval counts, the non-finite count (returned per thread)
template <int TI, bool COUNT>
__device__ __forceinline__ unsigned stage_chunk(const rovit_kan_stats& a, const Lds& l, int row0, int row_end, int i0, float inv_h0) {
  unsigned bad = 0;
  const int nk = a.n_knots;
  for (int p = threadIdx.x; p < SR * TI; p += NT) {
    const int r = p / TI, il = p % TI;
    const int row = row0 + r, i = i0 + il;
    float4 s0 = make_float4(0.f, __int_as_float(-1), 0.f, 0.f), s1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < row_end && i < a.in_f) {
      const float x = a.x[(size_t)row * a.in_f + i];
      const float xn = tanhf(x);
      const Basis4 b = kan_basis<false>(xn, l.knots, nk, inv_h0, nullptr);
      s0 = make_float4(x, __int_as_float(b.j), b.v[0], b.v[1]);
      s1 = make_float4(b.v[2], b.v[3], 0.f, 0.f);
      if (COUNT) {
        const int t = b.j >= 0 ? b.j : kan_interval(xn, l.knots, nk, inv_h0);
        atomicAdd(&l.occ[il * nk + t], 1u);
        bad += !isfinite(x);
      }
    }
    l.stage[2 * p] = s0;
    l.stage[2 * p + 1] = s1;
  }
  return bad;
}

// s and phi of one edge for one staged (row, input): the four live coefficients in a fixed order
__device__ __forceinline__ void edge_value(const float4 s0, const float4 s1, const float* wcol, int ow, float lw, float& s, float& phi) {
  const int t = __float_as_int(s0.y);
  s = 0.f;
  if (t >= 0) {
    s = s0.z * wcol[t * ow];
    s = fmaf(s0.w, wcol[max(t - 1, 0) * ow], s);
    s = fmaf(s1.x, wcol[max(t - 2, 0) * ow], s);
    s = fmaf(s1.y, wcol[max(t - 3, 0) * ow], s);
  }
  phi = fmaf(lw, s0.x, s);
}

// sum over the row groups in group order: red holds one value per thread; threads jo < ow of group 0 return the total
__device__ __forceinline__ double group_sum(double v, double* red, int ow, int rgs) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  double s = 0.0;
  if ((int)threadIdx.x < ow)
    for (int g = 0; g < rgs; ++g) s += red[g * ow + threadIdx.x];
  return s;
}

template <int TI>
__global__ __launch_bounds__(NT) void kan_edge_kernel(const rovit_kan_stats a, int ow, int chunks_per_split, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nk = a.n_knots, nb = nk - 4, tid = threadIdx.x;
  const Lds l = carve(smem, TI, nb, ow);
  const int i0 = blockIdx.x * TI, j0 = blockIdx.y * OT;
  const int jo = tid % ow, rg = tid / ow, rgs = NT / ow;
  const int j = j0 + jo;
  const bool live = j < a.out_f;
  if (tid < nk) l.knots[tid] = a.knots[tid];
  load_weight_tile<TI>(a, l.w, i0, j0, nb, ow);
  float lw[TI];
#pragma unroll
  for (int il = 0; il < TI; ++il) lw[il] = (live && i0 + il < a.in_f) ? a.lin_w[(size_t)j * a.in_f + i0 + il] : 0.f;
  __syncthreads();
  const float inv_h0 = 1.f / (l.knots[1] - l.knots[0]);
  double acc[TI][4];
#pragma unroll
  for (int il = 0; il < TI; ++il) acc[il][0] = acc[il][1] = acc[il][2] = acc[il][3] = 0.0;
  const int c0 = blockIdx.z * chunks_per_split;
  const long row_end = min((long)a.n, (long)(c0 + chunks_per_split) * SR);
  for (long row0 = (long)c0 * SR; row0 < row_end; row0 += SR) {
    __syncthreads();
    stage_chunk<TI, false>(a, l, (int)row0, (int)row_end, i0, inv_h0);
    __syncthreads();
    float f[TI][4];
#pragma unroll
    for (int il = 0; il < TI; ++il) f[il][0] = f[il][1] = f[il][2] = f[il][3] = 0.f;
#pragma unroll 4
    for (int t = 0; t < RPT; ++t) {
      const int r = rg + t * rgs;
      if (r >= SR) break;
#pragma unroll
      for (int il = 0; il < TI; ++il) {
        const float4 s0 = l.stage[2 * (r * TI + il)], s1 = l.stage[2 * (r * TI + il) + 1];
        float s, phi;
        edge_value(s0, s1, l.w + (size_t)il * nb * ow + jo, ow, lw[il], s, phi);
        f[il][0] += phi;
        f[il][1] = fmaf(phi, phi, f[il][1]);
        f[il][2] += fabsf(phi);
        f[il][3] += fabsf(s);
      }
    }
#pragma unroll
    for (int il = 0; il < TI; ++il)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[il][q] += (double)f[il][q];
  }
  const size_t E = (size_t)a.in_f * a.out_f;
  double* dst = part + (size_t)blockIdx.z * 4 * E;
#pragma unroll
  for (int il = 0; il < TI; ++il)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double s = group_sum(acc[il][q], l.red, ow, rgs);
      if (tid < ow && live && i0 + il < a.in_f) dst[q * E + (size_t)(i0 + il) * a.out_f + j] = s;
    }
}

template <int TI>
__global__ __launch_bounds__(NT) void kan_pre_kernel(const rovit_kan_stats a, int ow, double* __restrict__ part, int pp, size_t occ_word) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nk = a.n_knots, nb = nk - 4, tid = threadIdx.x;
  const Lds l = carve(smem, TI, nb, ow);
  const int j0 = blockIdx.y * OT;
  const int jo = tid % ow, rg = tid / ow, rgs = NT / ow;
  const int j = j0 + jo;
  const bool live = j < a.out_f, count = blockIdx.y == 0;
  const int row0 = blockIdx.x * SR;
  if (tid < nk) l.knots[tid] = a.knots[tid];
  __syncthreads();
  const float inv_h0 = 1.f / (l.knots[1] - l.knots[0]);
  float z[RPT];
  const float bias = live ? a.lin_b[j] : 0.f;
#pragma unroll
  for (int t = 0; t < RPT; ++t) z[t] = bias;
  unsigned bad = 0;
  double* dst = part + (size_t)blockIdx.x * pp;
  unsigned long long* res = reinterpret_cast<unsigned long long*>(a.result);
  for (int i0 = 0; i0 < a.in_f; i0 += TI) {
    __syncthreads();
    if (tid < TI * nk) l.occ[tid] = 0;
    load_weight_tile<TI>(a, l.w, i0, j0, nb, ow);
    float lw[TI];
#pragma unroll
    for (int il = 0; il < TI; ++il) lw[il] = (live && i0 + il < a.in_f) ? a.lin_w[(size_t)j * a.in_f + i0 + il] : 0.f;
    __syncthreads();
    if (count) bad += stage_chunk<TI, true>(a, l, row0, a.n, i0, inv_h0);
    else stage_chunk<TI, false>(a, l, row0, a.n, i0, inv_h0);
    __syncthreads();
    if (count) {
      if (tid < TI * nk && l.occ[tid] && i0 + tid / nk < a.in_f)
        atomicAdd(&res[occ_word + (size_t)(i0 + tid / nk) * nk + tid % nk], (unsigned long long)l.occ[tid]);
      if (tid >= NT - TI && i0 + (NT - 1 - tid) < a.in_f) {                 // sum |a_i| of the chunk in row order (rows beyond n staged as 0)
        const int il = NT - 1 - tid;
        double s = 0.0;
        for (int r = 0; r < SR; ++r) s += (double)fabsf(l.stage[2 * (r * TI + il)].x);
        dst[2 * a.out_f + i0 + il] = s;
      }
    }
#pragma unroll
    for (int t = 0; t < RPT; ++t) {
      const int r = rg + t * rgs;
      if (r < SR) {
#pragma unroll
        for (int il = 0; il < TI; ++il) {
          const float4 s0 = l.stage[2 * (r * TI + il)], s1 = l.stage[2 * (r * TI + il) + 1];
          float s, phi;
          edge_value(s0, s1, l.w + (size_t)il * nb * ow + jo, ow, lw[il], s, phi);
          z[t] += phi;
        }
      }
    }
  }
  double sz = 0.0, szz = 0.0;
#pragma unroll
  for (int t = 0; t < RPT; ++t) {
    const int r = rg + t * rgs;
    if (r < SR && row0 + r < a.n) {
      const double v = (double)z[t];
      sz += v;
      szz += v * v;
    }
  }
  const double tz = group_sum(sz, l.red, ow, rgs);
  if (tid < ow && live) dst[j] = tz;
  const double tzz = group_sum(szz, l.red, ow, rgs);
  if (tid < ow && live) dst[a.out_f + j] = tzz;
  if (count && bad) atomicAdd(&res[occ_word + (size_t)a.in_f * nk], (unsigned long long)bad);
}

__global__ __launch_bounds__(NT) void kan_fold_kernel(const rovit_kan_stats a, const double* __restrict__ part_edge, int splits,
                                                      const double* __restrict__ part_pre, int chunks, int pp) {
  const size_t E = (size_t)a.in_f * a.out_f, E4 = 4 * E, E5 = 5 * E;
  const size_t w = (size_t)blockIdx.x * NT + threadIdx.x;
  double* res = reinterpret_cast<double*>(a.result);
  if (w < E4) {
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += part_edge[(size_t)k * E4 + w];
    res[w] = s;
  } else if (w < E5) {                                              // the linear term's share of the edge: |w_ji| sum |a_i|
    const int i = (int)((w - E4) / a.out_f), j = (int)((w - E4) % a.out_f);
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part_pre[(size_t)c * pp + 2 * a.out_f + i];
    res[w] = fabs((double)a.lin_w[(size_t)j * a.in_f + i]) * s;
  } else if (w < E5 + pp) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part_pre[(size_t)c * pp + (w - E5)];
    res[w] = s;
  }
  if (w == 0) reinterpret_cast<long long*>(a.result)[E5 + pp + (size_t)a.in_f * a.n_knots + 1] = a.n;
}

// every edge's curve on the caller's grid xs (P points of the NORMALISED coordinate, no tanh: KANLayer.plot_activation's convention)
__global__ __launch_bounds__(NT) void kan_curves_kernel(const float* __restrict__ xs, const float* __restrict__ spline_w,
                                                        const float* __restrict__ knots, const float* __restrict__ lin_w, float* __restrict__ ys,
                                                        int in_f, int out_f, int nk, int P) {
  __shared__ float s_knots[KAN_MAX_KNOTS];
  if ((int)threadIdx.x < nk) s_knots[threadIdx.x] = knots[threadIdx.x];
  __syncthreads();
  const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (size_t)in_f * out_f * P) return;
  const int p = (int)(idx % P);
  const size_t e = idx / P;
  const int j = (int)(e % out_f), i = (int)(e / out_f), nb = nk - 4;
  const float x = xs[p];
  const Basis4 b = kan_basis<false>(x, s_knots, nk, 1.f / (s_knots[1] - s_knots[0]), nullptr);
  float s = 0.f;
  if (b.j >= 0) {
    const float* w = spline_w + e * nb;
    for (int m = 3; m >= 0; --m)                                   // ascending basis index, as a sum over the dense basis row runs
      if (b.j - m >= 0) s += b.v[m] * w[b.j - m];
  }
  if (lin_w) s += lin_w[(size_t)j * in_f + i] * x;
  ys[idx] = s;
}

static bool shape_ok(int in_f, int out_f, int nk) { return in_f >= 1 && out_f >= 1 && nk >= 5 && nk <= KAN_MAX_KNOTS; }

template <int TI>
static int launch_stats(const rovit_kan_stats* p, const Geometry& g, hipStream_t s) {
  const size_t E = (size_t)p->in_f * p->out_f;
  const int pp = 2 * p->out_f + p->in_f;
  double* part_edge = p->partials;
  double* part_pre = p->partials + (size_t)g.splits * 4 * E;
  hipLaunchKernelGGL(kan_edge_kernel<TI>, dim3(g.tiles, g.otiles, g.splits), dim3(NT), g.lds, s, *p, g.ow, g.chunks_per_split, part_edge);
  ROVIT_CHECK_LAUNCH("kan_edge_kernel");
  hipLaunchKernelGGL(kan_pre_kernel<TI>, dim3(g.chunks, g.otiles), dim3(NT), g.lds, s, *p, g.ow, part_pre, pp, 5 * E + pp);
  ROVIT_CHECK_LAUNCH("kan_pre_kernel");
  const size_t words = 5 * E + pp;
  hipLaunchKernelGGL(kan_fold_kernel, dim3((unsigned)((words + NT - 1) / NT)), dim3(NT), 0, s, *p, part_edge, g.splits, part_pre, g.chunks, pp);
  ROVIT_CHECK_LAUNCH("kan_fold_kernel");
  return ROVIT_OK;
}

}  // namespace

extern "C" size_t rovit_kan_stats_words(int in_f, int out_f, int n_knots) {
  if (!shape_ok(in_f, out_f, n_knots)) return 0;
  return 5 * (size_t)in_f * out_f + 2 * (size_t)out_f + in_f + (size_t)in_f * n_knots + 2;
}

extern "C" size_t rovit_kan_stats_partials_doubles(int n, int in_f, int out_f, int n_knots) {
  if (!shape_ok(in_f, out_f, n_knots) || n < 1) return 0;
  const Geometry g = geometry(n, in_f, out_f, n_knots);
  return (size_t)g.splits * 4 * in_f * out_f + (size_t)g.chunks * (2 * (size_t)out_f + in_f);
}

extern "C" int rovit_kan_edge_stats(const rovit_kan_stats* p, rovit_stream_t stream) {
  const char* who = "kan_edge_stats";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(shape_ok(p->in_f, p->out_f, p->n_knots), ROVIT_ERR_SHAPE, "%s: layer %d -> %d with %d knots (in, out >= 1; knots 5..%d)", who,
                  p->in_f, p->out_f, p->n_knots, KAN_MAX_KNOTS);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_KAN_STATS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_KAN_STATS_MAX_ROWS);
  ROVIT_CHECK_ARG((size_t)p->in_f * p->out_f <= ((size_t)1 << 26), ROVIT_ERR_SHAPE, "%s: %d x %d edges exceed 2^26", who, p->in_f, p->out_f);
  ROVIT_CHECK_ARG(p->x && p->spline_w && p->knots && p->lin_w && p->lin_b, ROVIT_ERR_NULL, "%s: an input or a parameter is missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->partials && p->result, ROVIT_ERR_NULL, "%s: the workspace or the result section is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->x, 4) && rovit_aligned(p->spline_w, 4) && rovit_aligned(p->knots, 4) && rovit_aligned(p->lin_w, 4) && rovit_aligned(p->lin_b, 4) &&
                      rovit_aligned(p->partials, 8) && rovit_aligned(p->result, 8),
                  ROVIT_ERR_ALIGN, "%s: a pointer is not aligned to its element size", who);
  const Geometry g = geometry(p->n, p->in_f, p->out_f, p->n_knots);
  ROVIT_CHECK_ARG(g.lds <= 64 * 1024, ROVIT_ERR_SHAPE, "%s: %zu bytes of LDS", who, g.lds);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(p->result, 0, rovit_kan_stats_words(p->in_f, p->out_f, p->n_knots) * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  if (g.ti == 4) return launch_stats<4>(p, g, s);
  if (g.ti == 2) return launch_stats<2>(p, g, s);
  return launch_stats<1>(p, g, s);
}

extern "C" int rovit_kan_curves(const float* xs, const float* spline_w, const float* knots, const float* lin_w, float* ys, int in_f, int out_f,
                                int n_knots, int num_points, rovit_stream_t stream) {
  const char* who = "kan_curves";
  ROVIT_CHECK_ARG(shape_ok(in_f, out_f, n_knots) && num_points >= 1, ROVIT_ERR_SHAPE, "%s: layer %d -> %d with %d knots, %d points", who, in_f, out_f,
                  n_knots, num_points);
  ROVIT_CHECK_ARG(xs && spline_w && knots && ys, ROVIT_ERR_NULL, "%s: the grid, a parameter or the output is missing (null pointer; lin_w alone may be)", who);
  ROVIT_CHECK_ARG(rovit_aligned(xs, 4) && rovit_aligned(spline_w, 4) && rovit_aligned(knots, 4) && rovit_aligned(lin_w, 4) && rovit_aligned(ys, 4), ROVIT_ERR_ALIGN,
                  "%s: a pointer is not aligned to its element size", who);
  const size_t total = (size_t)in_f * out_f * num_points;
  ROVIT_CHECK_ARG(total <= ((size_t)1 << 31), ROVIT_ERR_SHAPE, "%s: %zu values exceed 2^31", who, total);
  hipLaunchKernelGGL(kan_curves_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, xs, spline_w, knots, lin_w, ys,
                     in_f, out_f, n_knots, num_points);
  ROVIT_CHECK_LAUNCH("kan_curves_kernel");
  return ROVIT_OK;
}
