// Exact t-SNE (van der Maaten & Hinton 2008) of recorded feature rows on the device: the dense affinities P (rovit_tsne_affinities) and the
// gradient descent on the 2-D map (rovit_tsne_run).  All pairs, no tree and no neighbour list: at the few thousand to 16 k rows of this
// data set n^2 pairs per iteration are 10^7 .. 10^8 cheap interactions, P is read once per iteration, and the host never looks at the
// optimisation.  Definitions and limits: include/rovit_hip.h.
//
//   tsne_rows_kernel      a thread per row: the validity flag (every feature and the squared norm finite; with cosine the norm positive) and
//                         with cosine the unit row: the row scan of feature_tiles.h, the one neighbors.hip and kmeans.hip run.
//   tsne_dist_kernel      a 64 x 64 tile of D per work item; the two row tiles stream through LDS 32 features at a time; a thread owns a
//                         4 x 4 block and runs, per pair, ONE fp32 chain  acc = fma(x_ik - x_jk, x_ik - x_jk, acc), k ascending from 0: every
//                         term is non-negative, D_ii is 0 and D_ij = D_ji bit for bit.  Vector units, no matrix instruction: the difference
//                         form is no matrix product.
//   tsne_perp_kernel      a workgroup per row: the row of D staged once into LDS (64 KB at 16 384 rows), the minimum subtracted, 64 steps of
//                         the bisection on beta, then the conditional row written in place.
//   tsne_sym_kernel       tile pairs (a, b) and (b, a) through LDS, in place: P_ij = max((p_j|i + p_i|j) / (2 n_valid), 1e-12).
//   tsne_forces_kernel    a wave per two rows, eight rows per workgroup; y_j tiles in LDS; lanes stride over j, so P is read coalesced and
//                         once; a lane issues the loads of four columns and both rows together (3.8 TB/s of P at 16 384 rows against 3.0
//                         with one load in flight per row).  Per row the partial sums a, r, z (and A, B on the iterations that record
//                         the KL divergence).
//   tsne_update_kernel    every workgroup folds Z itself from the n partials (redundant, L2-resident), then the gains / momentum rule per
//                         element; workgroup 0 writes the KL divergence.
// Sums: a lane (or thread) adds its own elements in ascending index in fp32, the wave folds by the butterfly of wave_sum_t in fp32, waves
// are folded in wave order in fp64.  The element-to-lane map is a function of the index alone (j % 64, j % 256), never of the grid, so every
// output is the same bits for every max_workgroups.  No atomic of any kind; no kernel waits on another workgroup; two plain launches per
// iteration.
#include "common.h"
#include "feature_tiles.h"
#include "philox.h"

namespace {

constexpr int NT = 256;                          // threads per workgroup
constexpr int DT = 64;                           // rows and columns of a distance tile
constexpr int KC = 32;                           // features of one LDS chunk
constexpr int ST = 64;                           // rows and columns of a symmetrise tile
constexpr int FR = 8;                            // rows of a forces workgroup: two per wave
constexpr int FJ = 2048;                         // map rows of one LDS tile of the forces kernel
constexpr int FU = 4;                            // columns per lane whose loads of P are issued together
constexpr int PART_COLS = 8;                     // per-row partials, column-major (column c at c * n): a.x a.y r.x r.y z A B valid
constexpr int BISECTION_STEPS = 64;
constexpr float P_FLOOR = 1e-12f;

struct Layout { size_t ok, unconv, counts, mean, part, xhat, total; };
inline Layout layout_of(int n, int E) {
  Layout l;
  l.ok = 0;
  l.unconv = l.ok + rovit_up16((size_t)n * 4);
  l.counts = l.unconv + rovit_up16((size_t)n * 4);
  l.mean = l.counts + 16;
  l.part = l.mean + 16;
  l.xhat = l.part + rovit_up16((size_t)n * PART_COLS * 4);
  l.total = l.xhat + rovit_up16((size_t)n * E * 4);
  return l;
}

inline bool limits_ok(int n, int E) { return n >= 4 && n <= ROVIT_TSNE_MAX_ROWS && E >= 32 && E <= 256 && E % 32 == 0; }

// ---- fixed-order workgroup sums: fp32 inside the wave, fp64 across the four waves; two barriers, every thread must call -----------------
__device__ __forceinline__ double fold4(float v, double* s) {
  v = wave_sum_t(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = (double)v;
  __syncthreads();
  return ((s[0] + s[1]) + s[2]) + s[3];
}
__device__ __forceinline__ void fold4x2(float u, float v, double* s, double& U, double& V) {
  u = wave_sum_t(u);
  v = wave_sum_t(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    s[threadIdx.x >> 6] = (double)u;
    s[4 + (threadIdx.x >> 6)] = (double)v;
  }
  __syncthreads();
  U = ((s[0] + s[1]) + s[2]) + s[3];
  V = ((s[4] + s[5]) + s[6]) + s[7];
}
__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fminf(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

// ---- rows ------------------------------------------------------------------------------------------------------------------------------

struct RowArgs {
  int n, E, cosine;
  const float* x;
  int* ok;
  float* xhat;              // the unit rows with cosine, else nullptr
};

__global__ __launch_bounds__(NT) void tsne_rows_kernel(const RowArgs a) {
  const int chunks = (a.n + NT - 1) / NT;
  for (int w = blockIdx.x; w < chunks; w += gridDim.x) {
    const int row = w * NT + threadIdx.x;
    if (row >= a.n) continue;
    ftile::row_scan(a.x, nullptr, a.ok, a.xhat, row, a.E, a.cosine);   // the norm is not kept: the distances are of the difference form
  }
}

// one workgroup: the number of valid rows, for the symmetrise kernel
__global__ __launch_bounds__(NT) void tsne_count_kernel(int n, const int* ok, long long* counts) {
  __shared__ long long s[4];
  long long c = 0;
  for (int i = threadIdx.x; i < n; i += NT) c += ok[i] ? 1 : 0;
  c = block_sum_t<4>(c, s);
  if (threadIdx.x == 0) counts[0] = c;
}

// ---- distances -------------------------------------------------------------------------------------------------------------------------

struct DistArgs {
  int n, E, tiles;
  const float* x;
  const int* ok;
  float* D;
};

__global__ __launch_bounds__(NT) void tsne_dist_kernel(const DistArgs a) {
  __shared__ float As[DT][KC + 1];
  __shared__ float Bs[DT][KC + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long items = (long long)a.tiles * a.tiles;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int i0 = (int)(item / a.tiles) * DT, j0 = (int)(item % a.tiles) * DT;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int k0 = 0; k0 < a.E; k0 += KC) {
      __syncthreads();                                           // the previous chunk (or item) has been read
      for (int q = tid; q < DT * KC / 4; q += NT) {
        const int row = q / (KC / 4), c4 = q % (KC / 4), gi = i0 + row, gj = j0 + row;
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
        if (gi < a.n) u = *reinterpret_cast<const float4*>(a.x + (size_t)gi * a.E + k0 + 4 * c4);
        if (gj < a.n) v = *reinterpret_cast<const float4*>(a.x + (size_t)gj * a.E + k0 + 4 * c4);
        float* pa = &As[row][4 * c4];
        float* pb = &Bs[row][4 * c4];
        pa[0] = u.x; pa[1] = u.y; pa[2] = u.z; pa[3] = u.w;
        pb[0] = v.x; pb[1] = v.y; pb[2] = v.z; pb[3] = v.w;
      }
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < KC; ++k) {
        float av[4], bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = As[ty + 16 * r][k];
#pragma unroll
        for (int c = 0; c < 4; ++c) bv[c] = Bs[tx + 16 * c][k];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float d = av[r] - bv[c];
            acc[r][c] = fmaf(d, d, acc[r][c]);
          }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + ty + 16 * r;
      if (i >= a.n) continue;
      const bool iok = a.ok[i] != 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + tx + 16 * c;
        if (j < a.n) a.D[(size_t)i * a.n + j] = (iok && a.ok[j] != 0) ? acc[r][c] : 0.f;
      }
    }
  }
}

// ---- perplexity ------------------------------------------------------------------------------------------------------------------------

struct PerpArgs {
  int n;
  double log_perplexity;
  float* P;                 // D on entry, the conditional rows on exit
  const int* ok;
  float* beta;
  float* entropy;
  int* unconv;
};

__global__ __launch_bounds__(NT) void tsne_perp_kernel(const PerpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float row[];    // [n]: d - min for the row's candidates, -1 for the others
  __shared__ double s[8];
  __shared__ float s_min[4];
  const int tid = threadIdx.x, n = a.n;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    float* Pi = a.P + (size_t)i * n;
    const bool rowok = a.ok[i] != 0;
    float mn = __builtin_inff(), cnt = 0.f;
    __syncthreads();                                             // the previous row's s_min has been read
    for (int j = tid; j < n; j += NT) {
      const bool keep = rowok && j != i && a.ok[j] != 0;
      const float d = keep ? Pi[j] : -1.f;
      row[j] = d;
      if (keep) {
        mn = fminf(mn, d);
        cnt += 1.f;
      }
    }
    mn = wave_min_f(mn);
    if ((tid & 63) == 0) s_min[tid >> 6] = mn;
    const double count = fold4(cnt, s);                          // its barriers publish s_min too
    mn = fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));
    if (count < 1.0) {                                           // an invalid row, or no other valid row: an empty row (uniform branch)
      for (int j = tid; j < n; j += NT) Pi[j] = 0.f;
      if (tid == 0) {
        a.beta[i] = 0.f;
        a.entropy[i] = 0.f;
        a.unconv[i] = 0;
      }
      continue;
    }
    for (int j = tid; j < n; j += NT) {                          // a thread touches its own elements only: no barrier
      const float d = row[j];
      row[j] = d >= 0.f ? d - mn : -1.f;
    }
    double beta = 1.0, lo = 0.0, hi = 0.0, S = 1.0, H = 0.0;
    bool has_lo = false, has_hi = false;
    float bf = 1.f;
    for (int step = 0; step <= BISECTION_STEPS; ++step) {
      bf = (float)beta;
      float sw = 0.f, sdw = 0.f;
      for (int j = tid; j < n; j += NT) {
        const float d = row[j];
        if (d >= 0.f) {
          const float w = expf(-(bf * d));                       // d = 0 gives beta d = 0 for every finite beta: no 0 * inf
          sw += w;
          sdw = fmaf(d, w, sdw);
        }
      }
      double T;
      fold4x2(sw, sdw, s, S, T);
      H = log(S) + (double)bf * T / S;
      if (step == BISECTION_STEPS) break;
      if (H > a.log_perplexity) {
        lo = beta;
        has_lo = true;
        beta = has_hi ? 0.5 * (beta + hi) : beta * 2.0;
      } else {
        hi = beta;
        has_hi = true;
        beta = has_lo ? 0.5 * (beta + lo) : beta * 0.5;
      }
    }
    for (int j = tid; j < n; j += NT) {
      const float d = row[j];
      Pi[j] = d >= 0.f ? (float)((double)expf(-(bf * d)) / S) : 0.f;
    }
    if (tid == 0) {
      a.beta[i] = bf;
      a.entropy[i] = (float)H;
      a.unconv[i] = (has_lo && has_hi) ? 0 : 1;
    }
  }
}

// ---- symmetrise ------------------------------------------------------------------------------------------------------------------------

struct SymArgs {
  int n, tiles;
  float* P;
  const int* ok;
  const long long* counts;
};

__global__ __launch_bounds__(NT) void tsne_sym_kernel(const SymArgs a) {
  __shared__ float A[ST][ST + 1];
  __shared__ float B[ST][ST + 1];
  const int tid = threadIdx.x, n = a.n;
  const float den = 2.f * (float)a.counts[0];
  const long long items = (long long)a.tiles * a.tiles;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int ta = (int)(item / a.tiles), tb = (int)(item % a.tiles);
    if (ta > tb) continue;                                       // the pair is the work of (tb, ta); uniform
    const int a0 = ta * ST, b0 = tb * ST;
    const bool diag = ta == tb;
    __syncthreads();                                             // the previous item's tiles have been read
    for (int q = tid; q < ST * ST; q += NT) {
      const int r = q / ST, c = q % ST;
      A[r][c] = (a0 + r < n && b0 + c < n) ? a.P[(size_t)(a0 + r) * n + b0 + c] : 0.f;
      if (!diag) B[r][c] = (b0 + r < n && a0 + c < n) ? a.P[(size_t)(b0 + r) * n + a0 + c] : 0.f;
    }
    __syncthreads();                                             // both tiles are in LDS before either is overwritten in memory
    for (int q = tid; q < ST * ST; q += NT) {
      const int r = q / ST, c = q % ST;
      {
        const int gi = a0 + r, gj = b0 + c;
        if (gi < n && gj < n) {
          const float sum = A[r][c] + (diag ? A[c][r] : B[c][r]);
          a.P[(size_t)gi * n + gj] = (gi != gj && a.ok[gi] != 0 && a.ok[gj] != 0) ? fmaxf(sum / den, P_FLOOR) : 0.f;
        }
      }
      if (!diag) {
        const int gi = b0 + r, gj = a0 + c;
        if (gi < n && gj < n) {
          const float sum = B[r][c] + A[c][r];
          a.P[(size_t)gi * n + gj] = (a.ok[gi] != 0 && a.ok[gj] != 0) ? fmaxf(sum / den, P_FLOOR) : 0.f;
        }
      }
    }
  }
}

// one workgroup: the status words of the affinities
__global__ __launch_bounds__(NT) void tsne_affinity_status_kernel(int n, const int* ok, const int* unconv, const float* beta, long long* status) {
  __shared__ long long s[4];
  __shared__ float s_lo[4], s_hi[4];
  long long valid = 0, bad = 0;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int i = threadIdx.x; i < n; i += NT)
    if (ok[i]) {
      valid += 1;
      bad += unconv[i] ? 1 : 0;
      lo = fminf(lo, beta[i]);
      hi = fmaxf(hi, beta[i]);
    }
  valid = block_sum_t<4>(valid, s);
  bad = block_sum_t<4>(bad, s);
  lo = wave_min_f(lo);
  hi = wave_max_f(hi);
  if ((threadIdx.x & 63) == 0) {
    s_lo[threadIdx.x >> 6] = lo;
    s_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
    hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
    status[ROVIT_TSNE_N] = n;
    status[ROVIT_TSNE_N_VALID] = valid;
    status[ROVIT_TSNE_BAD_ROWS] = (long long)n - valid;
    status[ROVIT_TSNE_UNCONVERGED] = bad;
    status[ROVIT_TSNE_MIN_BETA] = (long long)__float_as_uint(lo);
    status[ROVIT_TSNE_MAX_BETA] = (long long)__float_as_uint(hi);
    status[6] = 0;
    status[7] = 0;
  }
}

// ---- the iteration ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool map_row_ok(float2 y) { return y.x == y.x && y.y == y.y; }   // a row with a NaN coordinate is absent

struct ForceArgs {
  int n, want_kl;
  const float* P;
  const float* Y;
  float* part;
};

__global__ __launch_bounds__(NT) void tsne_forces_kernel(const ForceArgs a) {
  __shared__ float2 ys[FJ];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = a.n;
  const float2* Y2 = reinterpret_cast<const float2*>(a.Y);
  const int groups = (n + FR - 1) / FR;
  for (int g = blockIdx.x; g < groups; g += gridDim.x) {
    int ri[2];
    float2 yi[2];
    bool iok[2];
    float ax[2], ay[2], rx[2], ry[2], z[2], A[2], B[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      ri[r] = g * FR + 2 * wv + r;
      yi[r] = ri[r] < n ? Y2[ri[r]] : make_float2(0.f, 0.f);
      iok[r] = ri[r] < n && map_row_ok(yi[r]);
      ax[r] = ay[r] = rx[r] = ry[r] = z[r] = A[r] = B[r] = 0.f;
    }
    for (int j0 = 0; j0 < n; j0 += FJ) {
      const int len = min(FJ, n - j0);
      __syncthreads();                                           // the previous tile has been read
      for (int q = tid; q < len; q += NT) ys[q] = Y2[j0 + q];
      __syncthreads();
      for (int jb = lane; jb < len; jb += 64 * FU) {
        float pv[FU][2];                                         // FU x 2 loads of P in flight before the first use
#pragma unroll
        for (int u = 0; u < FU; ++u)
#pragma unroll
          for (int r = 0; r < 2; ++r) pv[u][r] = (iok[r] && jb + 64 * u < len) ? a.P[(size_t)ri[r] * n + j0 + jb + 64 * u] : 0.f;
#pragma unroll
        for (int u = 0; u < FU; ++u) {                           // ascending j per lane, as without the batching: the same sums
          const int jj = jb + 64 * u, j = j0 + jj;
          if (jj < len) {
            const float2 yj = ys[jj];
            const bool jok = map_row_ok(yj);
#pragma unroll
            for (int r = 0; r < 2; ++r)
              if (iok[r]) {                                      // uniform over the wave
                const bool use = jok && j != ri[r];
                const float p = pv[u][r];
                const float dx = use ? yi[r].x - yj.x : 0.f, dy = use ? yi[r].y - yj.y : 0.f;
                const float q1 = 1.f + fmaf(dx, dx, dy * dy);
                const float w = use ? 1.f / q1 : 0.f;
                const float pw = p * w, ww = w * w;
                ax[r] = fmaf(pw, dx, ax[r]);
                ay[r] = fmaf(pw, dy, ay[r]);
                rx[r] = fmaf(ww, dx, rx[r]);
                ry[r] = fmaf(ww, dy, ry[r]);
                z[r] += w;
                if (a.want_kl && use && p > 0.f) {
                  A[r] = fmaf(p, logf(p) + logf(q1), A[r]);      // -log w = log(1 + |y_i - y_j|^2)
                  B[r] += p;
                }
              }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const float v[PART_COLS] = {wave_sum_t(ax[r]), wave_sum_t(ay[r]), wave_sum_t(rx[r]), wave_sum_t(ry[r]),
                                  wave_sum_t(z[r]),  wave_sum_t(A[r]),  wave_sum_t(B[r]),  iok[r] ? 1.f : 0.f};
      if (lane == 0 && ri[r] < n)
#pragma unroll
        for (int c = 0; c < PART_COLS; ++c) a.part[(size_t)c * n + ri[r]] = v[c];
    }
  }
}

struct UpdateArgs {
  int n, want_kl, trace_slot;
  float alpha, momentum, eta, auto_alpha;    // eta <= 0: max(n_valid / auto_alpha / 4, 50), n_valid counted here
  const float* part;
  float* Y;
  float* V;
  float* G;
  float* trace;
  float* grad_out;          // or nullptr
  float* z_out;             // or nullptr
};

__global__ __launch_bounds__(NT) void tsne_update_kernel(const UpdateArgs a) {
  __shared__ double s[8];
  const int tid = threadIdx.x, n = a.n;
  const float* zc = a.part + (size_t)4 * n;
  const float* vc = a.part + (size_t)7 * n;
  float zs = 0.f, cs = 0.f;
  for (int i = tid; i < n; i += NT) {
    zs += zc[i];
    cs += vc[i];                                                 // 0 / 1: exact in fp32 below 2^24
  }
  double Z, count;
  fold4x2(zs, cs, s, Z, count);
  const float Zf = (float)Z;
  const float eta = a.eta > 0.f ? a.eta : fmaxf((float)count / a.auto_alpha / 4.f, 50.f);
  for (long long e = (long long)blockIdx.x * NT + tid; e < 2ll * n; e += (long long)gridDim.x * NT) {
    const int i = (int)(e >> 1), c = (int)(e & 1);
    float g = 0.f;
    if (vc[i] != 0.f) {
      const float att = a.part[(size_t)c * n + i], rep = a.part[(size_t)(2 + c) * n + i];
      g = 4.f * (a.alpha * att - (Zf > 0.f ? rep / Zf : 0.f));
      float v = a.V[e], gain = a.G[e];
      gain = v * g < 0.f ? gain + 0.2f : gain * 0.8f;
      gain = fmaxf(gain, 0.01f);
      v = a.momentum * v - eta * gain * g;
      a.V[e] = v;
      a.G[e] = gain;
      a.Y[e] += v;
    }
    if (a.grad_out) a.grad_out[e] = g;
  }
  if (blockIdx.x == 0) {                                         // uniform over the workgroup
    if (a.want_kl) {
      const float* Ac = a.part + (size_t)5 * n;
      const float* Bc = a.part + (size_t)6 * n;
      float sa = 0.f, sb = 0.f;
      for (int i = tid; i < n; i += NT) {
        sa += Ac[i];
        sb += Bc[i];
      }
      double SA, SB;
      fold4x2(sa, sb, s, SA, SB);
      if (tid == 0) a.trace[a.trace_slot] = (float)(SA + log(Z) * SB);
    }
    if (tid == 0 && a.z_out) a.z_out[0] = Zf;
  }
}

// one workgroup: the mean of the valid rows of the map, and the status words of the run
__global__ __launch_bounds__(NT) void tsne_mean_kernel(int n, int n_iter, int n_trace, const float* Y, float* mean, long long* status) {
  __shared__ double s[8];
  const float2* Y2 = reinterpret_cast<const float2*>(Y);
  float sx = 0.f, sy = 0.f, cnt = 0.f, inf = 0.f;
  for (int i = threadIdx.x; i < n; i += NT) {
    const float2 y = Y2[i];
    if (map_row_ok(y)) {
      sx += y.x;
      sy += y.y;
      cnt += 1.f;
      inf += (isfinite(y.x) && isfinite(y.y)) ? 0.f : 1.f;
    }
  }
  double SX, SY, C, I;
  fold4x2(sx, sy, s, SX, SY);
  fold4x2(cnt, inf, s, C, I);
  if (threadIdx.x == 0) {
    mean[0] = C > 0.0 ? (float)(SX / C) : 0.f;
    mean[1] = C > 0.0 ? (float)(SY / C) : 0.f;
    status[ROVIT_TSNE_N] = n;
    status[ROVIT_TSNE_N_VALID] = (long long)C;
    status[ROVIT_TSNE_BAD_ROWS] = (long long)n - (long long)C;
    status[ROVIT_TSNE_RUN_ITERATIONS] = n_iter;
    status[ROVIT_TSNE_RUN_TRACE] = n_trace;
    status[ROVIT_TSNE_RUN_NONFINITE] = (long long)I;
    status[6] = 0;
    status[7] = 0;
  }
}

__global__ __launch_bounds__(NT) void tsne_center_kernel(int n, const float* mean, float* Y) {
  const float mx = mean[0], my = mean[1];
  for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < 2ll * n; e += (long long)gridDim.x * NT) Y[e] -= (e & 1) ? my : mx;
}

// 1e-4 x a standard normal per element: Box-Muller on words x and y of Philox(key = seed, counter = (element, 0, ROVIT_TSNE_STREAM, 0))
__global__ __launch_bounds__(NT) void tsne_random_kernel(unsigned long long seed, int count, float* Y) {
  for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < count; e += (long long)gridDim.x * NT) {
    const U4 c = philox4x32_10(seed, (unsigned)e, 0u, ROVIT_TSNE_STREAM, 0u);
    const float u1 = u01_open(c.x), u2 = u01(c.y);
    Y[e] = 1e-4f * (sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2));
  }
}

}  // namespace

extern "C" size_t rovit_tsne_workspace_bytes(int n, int embed) { return limits_ok(n, embed) ? layout_of(n, embed).total : 0; }

extern "C" int rovit_tsne_affinities(const rovit_tsne_affinity* p, rovit_stream_t stream) {
  const char* who = "tsne_affinities";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 4 && p->n <= ROVIT_TSNE_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (4..%d)", who, p->n, ROVIT_TSNE_MAX_ROWS);
  ROVIT_CHECK_ARG(p->embed >= 32 && p->embed <= 256 && p->embed % 32 == 0, ROVIT_ERR_SHAPE, "%s: embed %d (a multiple of 32 in 32..256)", who,
                  p->embed);
  ROVIT_CHECK_ARG(p->metric == ROVIT_KNN_L2 || p->metric == ROVIT_KNN_COSINE, ROVIT_ERR_SHAPE, "%s: metric %d", who, p->metric);
  ROVIT_CHECK_ARG(p->perplexity > 1.0 && p->perplexity < (double)(p->n - 1), ROVIT_ERR_SHAPE, "%s: perplexity %g (inside (1, n - 1) = (1, %d))", who,
                  p->perplexity, p->n - 1);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->features && p->workspace && p->P && p->beta && p->entropy && p->status, ROVIT_ERR_NULL, "%s: a null pointer", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->features) && rovit_aligned16(p->workspace) && rovit_aligned(p->P, 4) && rovit_aligned(p->beta, 4) &&
                      rovit_aligned(p->entropy, 4) && rovit_aligned(p->status, 8),
                  ROVIT_ERR_ALIGN, "%s: the rows or the workspace are not 16-byte aligned, or an array not to its words", who);
  const int n = p->n, E = p->embed;
  const Layout l = layout_of(n, E);
  ROVIT_CHECK_ARG(p->workspace_bytes >= l.total, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes,
                  l.total);
  const size_t perp_lds = (size_t)n * 4;
  ROVIT_CHECK_ARG(rovit_set_max_lds((const void*)tsne_perp_kernel, perp_lds), ROVIT_ERR_LAUNCH, "%s: cannot raise the LDS limit", who);
  char* ws = (char*)p->workspace;
  hipStream_t s = (hipStream_t)stream;
  const int mw = p->max_workgroups;
  const bool cosine = p->metric == ROVIT_KNN_COSINE;
  int* ok = (int*)(ws + l.ok);
  int* unconv = (int*)(ws + l.unconv);
  long long* counts = (long long*)(ws + l.counts);

  RowArgs ra;
  ra.n = n; ra.E = E; ra.cosine = cosine; ra.x = p->features; ra.ok = ok; ra.xhat = cosine ? (float*)(ws + l.xhat) : nullptr;
  hipLaunchKernelGGL(tsne_rows_kernel, rovit_grid((n + NT - 1) / NT, mw), dim3(NT), 0, s, ra);
  ROVIT_CHECK_LAUNCH("tsne_rows_kernel");
  hipLaunchKernelGGL(tsne_count_kernel, dim3(1), dim3(NT), 0, s, n, (const int*)ok, counts);
  ROVIT_CHECK_LAUNCH("tsne_count_kernel");

  DistArgs da;
  da.n = n; da.E = E; da.tiles = (n + DT - 1) / DT; da.x = cosine ? ra.xhat : p->features; da.ok = ok; da.D = p->P;
  hipLaunchKernelGGL(tsne_dist_kernel, rovit_grid((long long)da.tiles * da.tiles, mw), dim3(NT), 0, s, da);
  ROVIT_CHECK_LAUNCH("tsne_dist_kernel");
  if (p->distances_only) return ROVIT_OK;

  PerpArgs pa;
  pa.n = n; pa.log_perplexity = log(p->perplexity); pa.P = p->P; pa.ok = ok; pa.beta = p->beta; pa.entropy = p->entropy; pa.unconv = unconv;
  hipLaunchKernelGGL(tsne_perp_kernel, rovit_grid(n, mw), dim3(NT), perp_lds, s, pa);
  ROVIT_CHECK_LAUNCH("tsne_perp_kernel");

  if (p->symmetrize) {
    SymArgs sa;
    sa.n = n; sa.tiles = (n + ST - 1) / ST; sa.P = p->P; sa.ok = ok; sa.counts = counts;
    hipLaunchKernelGGL(tsne_sym_kernel, rovit_grid((long long)sa.tiles * sa.tiles, mw), dim3(NT), 0, s, sa);
    ROVIT_CHECK_LAUNCH("tsne_sym_kernel");
  }
  hipLaunchKernelGGL(tsne_affinity_status_kernel, dim3(1), dim3(NT), 0, s, n, (const int*)ok, (const int*)unconv, (const float*)p->beta,
                     (long long*)p->status);
  ROVIT_CHECK_LAUNCH("tsne_affinity_status_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_tsne_run(const rovit_tsne_descent* p, rovit_stream_t stream) {
  const char* who = "tsne_run";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 4 && p->n <= ROVIT_TSNE_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (4..%d)", who, p->n, ROVIT_TSNE_MAX_ROWS);
  ROVIT_CHECK_ARG(p->n_iter >= 1 && p->n_iter <= ROVIT_TSNE_MAX_ITER, ROVIT_ERR_SHAPE, "%s: %d iterations (1..%d)", who, p->n_iter,
                  ROVIT_TSNE_MAX_ITER);
  ROVIT_CHECK_ARG(p->exaggeration_iter >= 0 && p->kl_every >= 0 && p->max_workgroups >= 0, ROVIT_ERR_SHAPE,
                  "%s: exaggeration_iter %d, kl_every %d, max_workgroups %d (each >= 0)", who, p->exaggeration_iter, p->kl_every, p->max_workgroups);
  ROVIT_CHECK_ARG(p->early_exaggeration > 0.f && p->early_exaggeration < 1e30f, ROVIT_ERR_SHAPE, "%s: early_exaggeration %g (> 0)", who,
                  (double)p->early_exaggeration);
  ROVIT_CHECK_ARG(p->momentum_early >= 0.f && p->momentum_early < 1.f && p->momentum_late >= 0.f && p->momentum_late < 1.f, ROVIT_ERR_SHAPE,
                  "%s: momenta %g and %g (inside [0, 1))", who, (double)p->momentum_early, (double)p->momentum_late);
  ROVIT_CHECK_ARG(p->learning_rate == p->learning_rate && p->learning_rate < 1e30f, ROVIT_ERR_SHAPE, "%s: learning_rate %g", who,
                  (double)p->learning_rate);
  int slots = 0;
  if (p->kl_every > 0)
    for (int t = 0; t < p->n_iter; ++t) slots += (t % p->kl_every == 0 || t == p->n_iter - 1) ? 1 : 0;
  ROVIT_CHECK_ARG(p->trace_capacity >= slots, ROVIT_ERR_SHAPE, "%s: the trace holds %d values, %d are needed", who, p->trace_capacity, slots);
  ROVIT_CHECK_ARG(p->P && p->Y && p->V && p->G && p->workspace && p->status && (slots == 0 || p->trace), ROVIT_ERR_NULL, "%s: a null pointer", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->workspace) && rovit_aligned(p->P, 4) && rovit_aligned(p->Y, 8) && rovit_aligned(p->V, 4) &&
                      rovit_aligned(p->G, 4) && rovit_aligned(p->trace, 4) && rovit_aligned(p->status, 8) && rovit_aligned(p->grad_out, 4) &&
                      rovit_aligned(p->z_out, 4),
                  ROVIT_ERR_ALIGN, "%s: the workspace is not 16-byte aligned, the map not 8-byte aligned, or an array not to its words", who);
  const int n = p->n;
  const Layout l = layout_of(n, 32);                             // the sections in front of the unit rows do not depend on embed
  ROVIT_CHECK_ARG(p->workspace_bytes >= l.xhat, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes,
                  l.xhat);
  char* ws = (char*)p->workspace;
  hipStream_t s = (hipStream_t)stream;
  const int mw = p->max_workgroups;
  ForceArgs fa;
  fa.n = n; fa.P = p->P; fa.Y = p->Y; fa.part = (float*)(ws + l.part);
  UpdateArgs ua;
  ua.n = n; ua.eta = p->learning_rate; ua.auto_alpha = p->early_exaggeration; ua.part = fa.part;
  ua.Y = p->Y; ua.V = p->V; ua.G = p->G; ua.trace = p->trace; ua.grad_out = p->grad_out; ua.z_out = p->z_out;
  const dim3 fgrid = rovit_grid((n + FR - 1) / FR, mw), ugrid = rovit_grid((2ll * n + NT - 1) / NT, mw);
  int slot = 0;
  for (int t = 0; t < p->n_iter; ++t) {
    const bool early = t < p->exaggeration_iter;
    const int want_kl = (p->kl_every > 0 && (t % p->kl_every == 0 || t == p->n_iter - 1)) ? 1 : 0;
    fa.want_kl = want_kl;
    hipLaunchKernelGGL(tsne_forces_kernel, fgrid, dim3(NT), 0, s, fa);
    ROVIT_CHECK_LAUNCH("tsne_forces_kernel");
    ua.want_kl = want_kl; ua.trace_slot = slot;
    ua.alpha = early ? p->early_exaggeration : 1.f;
    ua.momentum = early ? p->momentum_early : p->momentum_late;
    hipLaunchKernelGGL(tsne_update_kernel, ugrid, dim3(NT), 0, s, ua);
    ROVIT_CHECK_LAUNCH("tsne_update_kernel");
    slot += want_kl;
  }
  hipLaunchKernelGGL(tsne_mean_kernel, dim3(1), dim3(NT), 0, s, n, p->n_iter, slots, (const float*)p->Y, (float*)(ws + l.mean),
                     (long long*)p->status);
  ROVIT_CHECK_LAUNCH("tsne_mean_kernel");
  if (p->center) {
    hipLaunchKernelGGL(tsne_center_kernel, ugrid, dim3(NT), 0, s, n, (const float*)(ws + l.mean), p->Y);
    ROVIT_CHECK_LAUNCH("tsne_center_kernel");
  }
  return ROVIT_OK;
}

extern "C" int rovit_tsne_random_init(unsigned long long seed, float* Y, int n, rovit_stream_t stream) {
  const char* who = "tsne_random_init";
  ROVIT_CHECK_ARG(n >= 1 && n <= ROVIT_TSNE_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, n, ROVIT_TSNE_MAX_ROWS);
  ROVIT_CHECK_ARG(Y, ROVIT_ERR_NULL, "%s: a null pointer", who);
  ROVIT_CHECK_ARG(rovit_aligned(Y, 4), ROVIT_ERR_ALIGN, "%s: the map is not aligned to its words", who);
  hipLaunchKernelGGL(tsne_random_kernel, rovit_grid((2ll * n + NT - 1) / NT, 0), dim3(NT), 0, (hipStream_t)stream, seed, 2 * n, Y);
  ROVIT_CHECK_LAUNCH("tsne_random_kernel");
  return ROVIT_OK;
}
