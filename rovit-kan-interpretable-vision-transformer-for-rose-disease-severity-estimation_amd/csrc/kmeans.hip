// k-means of the feature space on the device: k-means++ seeding, Lloyd iterations with the exact stopping rule, the per-cluster score
// card and the cluster x class contingency table (include/rovit_hip.h has the definitions).  The recipe `cdist` + `argmin` +
// `index_add_` materialises an (n, k) matrix, has no tie rule and sums its centroids with atomics; here no such matrix exists, the
// order is total, and every output is the same bits for every grid.
//
// Distance: the neighbours' (dist_of, feature_tiles.h): l2 = max(0, (|x|^2 + |c|^2) - 2 x.c), cosine = max(0, 1 - x^.c); every term fp32,
// x.c and the norms fma chains in ascending feature index.  The seeding kernel forms x.c with fmaf on the vector units, the assignment kernel on
// v_mfma_f32_32x32x2_f32, whose result is that chain: the same bits.  Order: the key (bits(d) << 32) | c, smallest first.
//
//   km_rows_kernel          a thread per row: squared norm, validity flag, with cosine the unit row; the counts (integer atomics).
//   km_seed_dist_kernel     a thread per row: the distance to the seed chosen by the previous pick (its index is read from device memory),
//                           the running minimum, and the maximum of the minima as an integer maximum of the bits (d >= 0).
//   km_seed_weights_kernel  w_i = floor(d_i 2^(40 - e)) as 64-bit integers, the sums and the valid counts of every 256-row block.
//   km_seed_pick_kernel     one workgroup: W, t = floor(r64 W / 2^64), the block that holds t, the row inside it; copies the row out.
//   km_assign_kernel        a work item = a tile of 64 rows.  The centroids sit in LDS in the search kernel's (f0 f2 f4 f6 | f1 f3 f5 f7)
//                           group layout: k <= 64 for the whole launch, a larger k in 64-centroid tiles.  Wave (qt, ct) forms the 32 x 32
//                           block of row sub-tile qt against centroid sub-tile ct with the rows on the lane index: a lane holds 16 centroid
//                           distances of ONE row and keeps its two smallest keys in registers.  The four pairs of a row (two lane halves,
//                           two waves) meet in LDS; a thread per row takes the two smallest and writes label, distance, second distance
//                           and silhouette.  The changed-row count is a wave ballot and one integer atomic per wave.
//   km_count / km_scan / km_scatter_kernel   the two-level counting sort of the rows by label: per 256-row block counts (LDS integer
//                           atomics), per cluster an exclusive scan over the blocks, then every row's slot = cluster offset + block base +
//                           its rank among the block's earlier rows of the same label: members in ascending row index.
//   km_partial_kernel       a work item = a segment of 1024 members of one cluster: a thread per feature adds the members in order in fp64;
//                           the segment's inertia and silhouette shares, medoid key and radius.
//   km_finalize_kernel      a workgroup per cluster: the segments in ascending order, the mean, the rounding (update), or the cluster's
//                           line of the status block (final pass).  It also owns the stopping flag.
//   km_contingency_kernel   integer atomics into the (k, C) table.
// A run enqueues max_iter iterations at once; every kernel of an iteration returns at once when the flag is set.
#include "common.h"
#include "feature_tiles.h"
#include "philox.h"
#include "topk_device.h"

namespace {

using namespace ftile;                           // row_scan, count_rows, store_unit, tile_dot, acc_row, dist_of
using namespace topk;                            // u64, EMPTY, key_of, key_bits, key_index

constexpr int NT = 256;                          // threads per workgroup = rows of a sort block
constexpr int QT = 64, CT = 64;                  // rows / centroids of an LDS tile
constexpr int MAX_T = 8;                         // embed / 32
constexpr int MAXK = ROVIT_KMEANS_MAX_K;
constexpr int SEG = ROVIT_KMEANS_SEGMENT;
constexpr int ASSIGN_WGS = 512;                  // workgroups of the assignment launch (the result does not depend on it)
static_assert(NT == MAXK, "a thread per cluster in the count kernel");
static_assert(SEG % NT == 0, "a segment is a whole number of passes of the workgroup");

enum { S_DMAX = 0, S_WORDS = 16 };               // the workspace's scalar section (8-byte words)

struct Layout { size_t norm, ok, mind, cnorm, blockw, blockv, cnt, base, total, order, psum, pst, scal, bytes; int nb, nseg; };
inline Layout layout_of(int n, int E, int k) {
  Layout l;
  l.nb = (n + NT - 1) / NT;
  l.nseg = (n + SEG - 1) / SEG + k;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += rovit_up16(bytes); return at; };
  l.norm = take((size_t)n * 4);
  l.ok = take((size_t)n * 4);
  l.mind = take((size_t)n * 4);
  l.cnorm = take((size_t)MAXK * 4);
  l.blockw = take((size_t)l.nb * 8);
  l.blockv = take((size_t)l.nb * 8);
  l.cnt = take((size_t)l.nb * k * 4);
  l.base = take((size_t)l.nb * k * 4);
  l.total = take((size_t)MAXK * 4);
  l.order = take((size_t)n * 4);
  l.psum = take((size_t)l.nseg * E * 8);
  l.pst = take((size_t)l.nseg * 4 * 8);
  l.scal = take((size_t)S_WORDS * 8);
  l.bytes = o;
  return l;
}

inline bool limits_ok(int n, int E, int k) {
  return n >= 1 && n <= ROVIT_KMEANS_MAX_ROWS && E >= 32 && E <= 256 && E % 32 == 0 && k >= 1 && k <= MAXK;
}

// ---- rows: norms, flags, the unit rows ----------------------------------------------------------------------------------------------------

struct RowArgs {
  int n, E, cosine;
  const float* x;
  float* norm;
  int* ok;
  float* xhat;              // or nullptr
  u64* status;
};

__global__ __launch_bounds__(NT) void km_rows_kernel(const RowArgs a) {
  const int chunks = (a.n + NT - 1) / NT;
  for (int w = blockIdx.x; w < chunks; w += gridDim.x) {
    const int row = w * NT + threadIdx.x;
    bool good = false;
    if (row < a.n) good = row_scan(a.x, a.norm, a.ok, a.xhat, row, a.E, a.cosine);
    count_rows(a.status, good, row, a.n, ROVIT_KMEANS_N, ROVIT_KMEANS_N_VALID, ROVIT_KMEANS_BAD_ROWS);
  }
}

// |c|^2 of every centroid: the rows' chain
__global__ __launch_bounds__(NT) void km_cnorm_kernel(const float* c, float* cn, int k, int E) {
  const int j = blockIdx.x * NT + threadIdx.x;
  if (j >= k) return;
  float s = 0.f;
  for (int f = 0; f < E; ++f) s = fmaf(c[(size_t)j * E + f], c[(size_t)j * E + f], s);
  cn[j] = s;
}

// ---- seeding ----------------------------------------------------------------------------------------------------------------------------

struct SeedArgs {
  int n, E, cosine, j, restart;
  unsigned long long seed;
  const float* x;           // the rows the distances are taken on (the unit rows with cosine)
  const float* norm;
  const int* ok;
  float* mind;
  u64* blockw;
  u64* blockv;
  unsigned* dmax;
  int* seeds;
  float* centroids;
  float* cnorm;
  float* tap;               // or nullptr
  u64* status;
};

__device__ __forceinline__ u64 weight_of(float d, int e) {
  return d < __builtin_inff() ? (u64)ldexp((double)d, 40 - e) : 0ull;      // exact: a power-of-two scaling of an fp32 value, d < 2^e
}

__global__ __launch_bounds__(NT) void km_seed_dist_kernel(const SeedArgs a) {      // j >= 1
  const int chunks = (a.n + NT - 1) / NT, E4 = a.E / 4;
  const int chosen = a.seeds[a.j - 1];
  unsigned mx = 0u;
  for (int w = blockIdx.x; w < chunks; w += gridDim.x) {
    const int row = w * NT + threadIdx.x;
    if (row < a.n && a.ok[row]) {
      float d = 0.f;
      if (chosen >= 0 && chosen < a.n) {
        const float4* xr = reinterpret_cast<const float4*>(a.x + (size_t)row * a.E);
        const float4* cr = reinterpret_cast<const float4*>(a.x + (size_t)chosen * a.E);
        float dot = 0.f;
        for (int c = 0; c < E4; ++c) {
          const float4 u = xr[c], v = cr[c];
          dot = fmaf(u.x, v.x, dot);
          dot = fmaf(u.y, v.y, dot);
          dot = fmaf(u.z, v.z, dot);
          dot = fmaf(u.w, v.w, dot);
        }
        bool fin;
        d = dist_of(a.cosine, a.norm[row], a.norm[chosen], dot, &fin);
      }
      if (a.j > 1) d = fminf(a.mind[row], d);
      a.mind[row] = d;
      const unsigned b = __float_as_uint(d);
      mx = b > mx ? b : mx;
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned o = __shfl_xor(mx, m);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(a.dmax, mx);
}

__device__ __forceinline__ int exponent_of(float dmax) {
  int e = 0;
  if (dmax > 0.f && dmax < __builtin_inff()) frexpf(dmax, &e);
  return e;
}

__global__ __launch_bounds__(NT) void km_seed_weights_kernel(const SeedArgs a) {
  __shared__ u64 s_sum[4];
  const int chunks = (a.n + NT - 1) / NT;
  const float dmax = __uint_as_float(*a.dmax);
  const bool uniform = a.j == 0 || !(dmax > 0.f);
  const int e = exponent_of(dmax);
  for (int w = blockIdx.x; w < chunks; w += gridDim.x) {
    const int row = w * NT + threadIdx.x;
    const bool valid = row < a.n && a.ok[row] != 0;
    const float d = (valid && a.j > 0) ? a.mind[row] : 0.f;
    if (a.tap && a.j > 0 && row < a.n) a.tap[(size_t)a.j * a.n + row] = valid ? d : __builtin_inff();
    const u64 wt = (valid && !uniform) ? weight_of(d, e) : 0ull;
    const u64 sw = block_sum_t<4>(wt, s_sum);
    const u64 sv = block_sum_t<4>((u64)(valid ? 1 : 0), s_sum);
    if (threadIdx.x == 0) {
      a.blockw[w] = sw;
      a.blockv[w] = sv;
    }
  }
}

__global__ __launch_bounds__(NT) void km_seed_pick_kernel(const SeedArgs a) {      // one workgroup
  __shared__ u64 s_sum[4];
  __shared__ u64 s_w[NT];
  __shared__ u64 s_pre[NT];
  __shared__ long long s_pick[2];
  __shared__ int s_row;
  const int tid = threadIdx.x, nb = (a.n + NT - 1) / NT, per = (nb + NT - 1) / NT;
  const int b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
  u64 lw = 0, lv = 0;
  for (int b = b0; b < b1; ++b) {
    lw += a.blockw[b];
    lv += a.blockv[b];
  }
  const u64 W = block_sum_t<4>(lw, s_sum), V = block_sum_t<4>(lv, s_sum);
  const bool uniform = a.j == 0 || W == 0;
  const u64 total = uniform ? V : W, mine = uniform ? lv : lw;
  const u64* bw = uniform ? a.blockv : a.blockw;
  const int e = exponent_of(__uint_as_float(*a.dmax));
  if (tid == 0) {
    s_row = -1;
    s_pick[0] = 0;
    s_pick[1] = 0;
  }
  s_w[tid] = mine;
  __syncthreads();
  if (tid == 0) {
    u64 run = 0;
    for (int i = 0; i < NT; ++i) {
      s_pre[i] = run;
      run += s_w[i];
    }
  }
  __syncthreads();
  if (total > 0) {                                                // uniform over the workgroup
    const U4 r = philox4x32_10(a.seed, (unsigned)a.j, (unsigned)a.restart, ROVIT_KMEANS_STREAM, 0u);
    const u64 r64 = ((u64)r.x << 32) | (u64)r.y;
    const u64 t = __umul64hi(r64, total);                          // floor(r64 total / 2^64) < total
    const u64 pre = s_pre[tid];
    if (t >= pre && t < pre + mine) {                              // exactly one thread
      u64 run = pre;
      for (int b = b0; b < b1; ++b) {
        const u64 v = bw[b];
        if (t < run + v) {
          s_pick[0] = b;
          s_pick[1] = (long long)(t - run);
          break;
        }
        run += v;
      }
    }
    __syncthreads();
    const int b = (int)s_pick[0];
    const u64 resid = (u64)s_pick[1];
    const int row = b * NT + tid;
    const bool valid = row < a.n && a.ok[row] != 0;
    s_w[tid] = !valid ? 0ull : (uniform ? 1ull : weight_of(a.mind[row], e));
    __syncthreads();
    if (tid == 0) {
      u64 run = 0;
      for (int i = 0; i < NT; ++i) {
        run += s_w[i];
        if (run > resid) {
          s_row = b * NT + i;
          break;
        }
      }
    }
    __syncthreads();
  }
  const int row = s_row;                                          // < n: a row with a positive weight
  if (tid < a.E) a.centroids[(size_t)a.j * a.E + tid] = row >= 0 ? a.x[(size_t)row * a.E + tid] : 0.f;
  if (tid == 0) {
    a.seeds[a.j] = row;
    a.cnorm[a.j] = row >= 0 ? a.norm[row] : 0.f;
    if (a.j > 0 && W == 0) a.status[ROVIT_KMEANS_W0_EVENTS] += 1;
    if ((u64)(a.j + 1) > V) a.status[ROVIT_KMEANS_SHORT] = 1;
    *a.dmax = 0u;
  }
}

// ---- assignment -------------------------------------------------------------------------------------------------------------------------

struct AssignArgs {
  int n, E, k, cosine, force, parity;
  const float* x;           // the rows (the unit rows with cosine)
  const float* xn;
  const int* ok;
  const float* c;
  const float* cn;
  int* labels;
  float* d1;
  float* d2;
  float* sil;
  u64* status;
};

inline size_t assign_lds_bytes(int E) { return ((size_t)(QT + CT) * (E + 4) + CT) * 4 + (size_t)QT * 8 * 8; }

__device__ __forceinline__ void two_insert(u64& k1, u64& k2, u64 key) {
  const u64 lo = key < k1 ? key : k1, hi = key < k1 ? k1 : key;
  k1 = lo;
  k2 = hi < k2 ? hi : k2;
}

__global__ __launch_bounds__(NT) void km_assign_kernel(const AssignArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (!a.force && a.status[ROVIT_KMEANS_DONE] != 0) return;
  const int E = a.E, ST = E + 4, E8 = E / 8, T = E / 32;
  float* Qs = lds;                                               // [64][ST] rows
  float* Cs = Qs + QT * ST;                                      // [64][ST] one centroid tile
  float* s_cn = Cs + CT * ST;                                    // [64] squared norms of the tile's centroids
  u64* Ms = reinterpret_cast<u64*>(s_cn + CT);                   // [64][4][2] the key pairs of a tile's rows
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), qtw = wv >> 1, ctw = wv & 1;
  const int tiles = (a.n + QT - 1) / QT, ctiles = (a.k + CT - 1) / CT;
  auto stage_centroids = [&](int ct) {                           // store_unit's order: k ascending in feature index, as for the rows below
#pragma unroll
    for (int i = 0; i < MAX_T; ++i)
      if (i < T) {
        const int idx = tid + NT * i, row = idx / E8, c8 = idx - row * E8, cc = ct * CT + row;
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
        if (cc < a.k) {
          const float4* src = reinterpret_cast<const float4*>(a.c + (size_t)cc * E + 8 * c8);
          u = src[0];
          v = src[1];
        }
        store_unit(Cs + row * ST + 8 * c8, u, v);
      }
    if (tid < CT) {
      const int cc = ct * CT + tid;
      s_cn[tid] = (cc < a.k && !a.cosine) ? a.cn[cc] : 0.f;
    }
  };
  if (ctiles == 1) stage_centroids(0);                           // resident for the whole launch; published by the loop's barriers
  float4 pu[MAX_T], pv[MAX_T];
  int p_ok[MAX_T];
  auto fetch = [&](int item) {                                   // a row tile into registers; the flags are applied when it is staged
#pragma unroll
    for (int i = 0; i < MAX_T; ++i)
      if (i < T) {
        const int idx = tid + NT * i, row = idx / E8, c8 = idx - row * E8, g = item * QT + row;
        pu[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        pv[i] = pu[i];
        p_ok[i] = 0;
        if (g < a.n) {
          const float4* src = reinterpret_cast<const float4*>(a.x + (size_t)g * E + 8 * c8);
          pu[i] = src[0];
          pv[i] = src[1];
          p_ok[i] = a.ok[g];
        }
      }
  };
  if ((int)blockIdx.x < tiles) fetch(blockIdx.x);
  for (int item = blockIdx.x; item < tiles; item += gridDim.x) {
    const int q0 = item * QT;
    __syncthreads();                                             // the previous item's products and pairs have been read
#pragma unroll
    for (int i = 0; i < MAX_T; ++i)
      if (i < T) {
        const int idx = tid + NT * i, row = idx / E8, c8 = idx - row * E8;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        store_unit(Qs + row * ST + 8 * c8, p_ok[i] ? pu[i] : z, p_ok[i] ? pv[i] : z);
      }
    if (item + (int)gridDim.x < tiles) fetch(item + gridDim.x);   // in flight behind the products below
    const int qrow = q0 + qtw * 32 + l31;
    const bool qgood = qrow < a.n && a.ok[qrow] != 0;
    const float qn = qgood ? a.xn[qrow] : 0.f;
    u64 k1 = EMPTY, k2 = EMPTY;
    for (int ct = 0; ct < ctiles; ++ct) {
      if (ctiles > 1) {
        __syncthreads();                                         // the previous tile's products are done
        stage_centroids(ct);
      }
      __syncthreads();
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* crow = Cs + (ctw * 32 + l31) * ST + 4 * lh;   // A[m = centroid][k]: lane half h holds feature 8 b + 2 s + h in step s
      const float* qrw = Qs + (qtw * 32 + l31) * ST + 4 * lh;    // B[k][n = row]
      acc = tile_dot(acc, crow, qrw, E);
      // lane (l31, h) holds x.c of row l31 against the sub-tile's centroids acc_row(r, h)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = ctw * 32 + acc_row(r, lh), cc = ct * CT + i;
        bool fin;
        const float d = dist_of(a.cosine, qn, s_cn[i], acc[r], &fin);
        const u64 key = (qgood && cc < a.k && fin) ? key_of(__float_as_uint(d), cc) : EMPTY;
        two_insert(k1, k2, key);
      }
    }
    {
      u64* mine = Ms + ((qtw * 32 + l31) * 4 + ctw * 2 + lh) * 2;
      mine[0] = k1;
      mine[1] = k2;
    }
    __syncthreads();
    if (tid < QT) {                                              // wave 0: a thread per row of the tile
      const int g = q0 + tid;
      bool changed = false;
      if (g < a.n) {
        const u64* base = Ms + tid * 8;
        u64 b1 = EMPTY, b2 = EMPTY;
#pragma unroll
        for (int i = 0; i < 8; ++i) two_insert(b1, b2, base[i]);
        const int label = b1 != EMPTY ? key_index(b1) : -1;
        const float d1 = b1 != EMPTY ? __uint_as_float(key_bits(b1)) : __builtin_inff();
        const float d2 = b2 != EMPTY ? __uint_as_float(key_bits(b2)) : __builtin_inff();
        float sil = 0.f;
        if (b2 != EMPTY) {
          const float sa = a.cosine ? d1 : sqrtf(d1), sb = a.cosine ? d2 : sqrtf(d2), mx = sa > sb ? sa : sb;
          sil = mx > 0.f ? (sb - sa) / mx : 0.f;
        }
        changed = a.labels[g] != label;
        a.labels[g] = label;
        a.d1[g] = d1;
        a.d2[g] = d2;
        a.sil[g] = sil;
      }
      const u64 m = __ballot(changed);
      if (tid == 0 && m) atomicAdd(&a.status[ROVIT_KMEANS_CHANGED + a.parity], (u64)__popcll(m));
    }
  }
}

// ---- the counting sort by label ---------------------------------------------------------------------------------------------------------

struct SortArgs {
  int n, k, it, force;
  const int* labels;
  int* cnt;                 // (blocks, k)
  int* base;                // (blocks, k)
  int* total;               // (k)
  int* order;               // (n)
  const u64* status;
};

__device__ __forceinline__ bool km_skip(const u64* status, int force, int it) {
  return !force && (status[ROVIT_KMEANS_DONE] != 0 || status[ROVIT_KMEANS_CHANGED + (it & 1)] == 0);
}

__global__ __launch_bounds__(NT) void km_count_kernel(const SortArgs a) {
  __shared__ int h[MAXK];
  if (km_skip(a.status, a.force, a.it)) return;
  const int nb = (a.n + NT - 1) / NT, tid = threadIdx.x;
  for (int b = blockIdx.x; b < nb; b += gridDim.x) {
    h[tid] = 0;
    __syncthreads();
    const int row = b * NT + tid;
    if (row < a.n) {
      const int l = a.labels[row];
      if (l >= 0 && l < a.k) atomicAdd(&h[l], 1);
    }
    __syncthreads();
    if (tid < a.k) a.cnt[(size_t)b * a.k + tid] = h[tid];         // the thread that reads h[tid] is the one that clears it
  }
}

__global__ __launch_bounds__(NT) void km_scan_kernel(const SortArgs a) {           // a workgroup per cluster
  __shared__ int s_w[NT];
  if (km_skip(a.status, a.force, a.it)) return;
  const int nb = (a.n + NT - 1) / NT, tid = threadIdx.x, per = (nb + NT - 1) / NT;
  const int b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
  for (int c = blockIdx.x; c < a.k; c += gridDim.x) {
    int local = 0;
    for (int b = b0; b < b1; ++b) local += a.cnt[(size_t)b * a.k + c];
    __syncthreads();                                             // the previous cluster's sums have been read
    s_w[tid] = local;
    __syncthreads();
    int run = 0;
    for (int i = 0; i < tid; ++i) run += s_w[i];
    if (tid == NT - 1) a.total[c] = run + local;
    for (int b = b0; b < b1; ++b) {
      a.base[(size_t)b * a.k + c] = run;
      run += a.cnt[(size_t)b * a.k + c];
    }
  }
}

__global__ __launch_bounds__(NT) void km_scatter_kernel(const SortArgs a) {
  __shared__ int s_l[NT];
  __shared__ int s_off[MAXK];
  if (km_skip(a.status, a.force, a.it)) return;
  const int nb = (a.n + NT - 1) / NT, tid = threadIdx.x;
  if (tid == 0) {
    int run = 0;
    for (int c = 0; c < a.k; ++c) {
      s_off[c] = run;
      run += a.total[c];
    }
  }
  for (int b = blockIdx.x; b < nb; b += gridDim.x) {
    const int row = b * NT + tid;
    int l = row < a.n ? a.labels[row] : -1;
    if (l >= a.k) l = -1;
    __syncthreads();                                             // the previous block's labels have been read; s_off is published
    s_l[tid] = l;
    __syncthreads();
    if (l >= 0) {
      int rank = 0;
      for (int s = 0; s < tid; ++s) rank += s_l[s] == l ? 1 : 0;
      a.order[s_off[l] + a.base[(size_t)b * a.k + l] + rank] = row;   // < the number of labelled rows <= n
    }
  }
}

// ---- update and score card --------------------------------------------------------------------------------------------------------------

struct UpdArgs {
  int n, E, k, cosine, it, force, stats, max_iter;
  const float* x;           // the rows (the unit rows with cosine)
  const int* order;
  const int* total;
  const float* d1;
  const float* sil;
  double* psum;             // (segments, E)
  u64* pst;                 // (segments, 4): inertia, silhouette (fp64 bits), medoid key, radius bits
  float* c;
  float* cn;
  u64* status;
};

// segment and member offsets of every cluster, by one thread (k <= 256)
__device__ __forceinline__ void km_offsets(const int* total, int k, int* s_seg, int* s_off) {
  if (threadIdx.x == 0) {
    int seg = 0, off = 0;
    for (int c = 0; c < k; ++c) {
      s_seg[c] = seg;
      s_off[c] = off;
      seg += (total[c] + SEG - 1) / SEG;
      off += total[c];
    }
    s_seg[k] = seg;
    s_off[k] = off;
  }
  __syncthreads();
}

__global__ __launch_bounds__(NT) void km_partial_kernel(const UpdArgs a) {
  __shared__ int s_seg[MAXK + 1];
  __shared__ int s_off[MAXK + 1];
  __shared__ double s_d[4];
  __shared__ u64 s_u[8];
  if (km_skip(a.status, a.force, a.it)) return;
  const int tid = threadIdx.x;
  km_offsets(a.total, a.k, s_seg, s_off);
  const int nsegs = s_seg[a.k];                                  // <= ceil(n / SEG) + k, the workspace's segment count
  for (int g = blockIdx.x; g < nsegs; g += gridDim.x) {
    int lo = 0, hi = a.k - 1;
    while (lo < hi) {                                            // the first cluster whose segments end above g
      const int mid = (lo + hi) >> 1;
      if (s_seg[mid + 1] <= g) lo = mid + 1; else hi = mid;
    }
    const int c = lo, m0 = s_off[c] + (g - s_seg[c]) * SEG, m1 = min(s_off[c + 1], m0 + SEG);
    if (tid < a.E) {
      double acc = 0.0;
      int m = m0;
      for (; m + 8 <= m1; m += 8) {                               // eight loads in flight; added in member order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = a.x[(size_t)a.order[m + u] * a.E + tid];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (double)v[u];
      }
      for (; m < m1; ++m) acc += (double)a.x[(size_t)a.order[m] * a.E + tid];
      a.psum[(size_t)g * a.E + tid] = acc;
    }
    double in = 0.0, sl = 0.0;
    u64 key = EMPTY;
    unsigned rad = 0u;
    for (int m = m0 + tid; m < m1; m += NT) {
      const int r = a.order[m];
      const float d = a.d1[r];
      const unsigned bits = __float_as_uint(d);
      in += (double)d;
      sl += (double)a.sil[r];
      const u64 kk = key_of(bits, r);
      key = kk < key ? kk : key;
      rad = bits > rad ? bits : rad;
    }
    in = block_sum_t<4>(in, s_d);
    sl = block_sum_t<4>(sl, s_d);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const u64 ok = __shfl_xor(key, m);
      const unsigned orr = __shfl_xor(rad, m);
      key = ok < key ? ok : key;
      rad = orr > rad ? orr : rad;
    }
    __syncthreads();
    if ((tid & 63) == 0) {
      s_u[tid >> 6] = key;
      s_u[4 + (tid >> 6)] = rad;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w) {
        key = s_u[w] < key ? s_u[w] : key;
        rad = (unsigned)s_u[4 + w] > rad ? (unsigned)s_u[4 + w] : rad;
      }
      u64* o = a.pst + (size_t)g * 4;
      o[0] = (u64)__double_as_longlong(in);
      o[1] = (u64)__double_as_longlong(sl);
      o[2] = key;
      o[3] = rad;
    }
  }
}

__global__ __launch_bounds__(NT) void km_finalize_kernel(const UpdArgs a) {        // a workgroup per cluster
  __shared__ int s_seg[MAXK + 1];
  __shared__ int s_off[MAXK + 1];
  __shared__ double s_m[NT];
  __shared__ float s_c[NT];
  const int tid = threadIdx.x;
  if (!a.force) {
    if (a.status[ROVIT_KMEANS_DONE] != 0) return;
    if (a.status[ROVIT_KMEANS_CHANGED + (a.it & 1)] == 0) {       // no label changed: the run is over; every workgroup sees the same word
      if (blockIdx.x == 0 && tid == 0) {
        a.status[ROVIT_KMEANS_DONE] = 1;
        a.status[ROVIT_KMEANS_N_ITER] = (u64)a.it;
      }
      return;
    }
    if (blockIdx.x == 0 && tid == 0) a.status[ROVIT_KMEANS_CHANGED + ((a.it + 1) & 1)] = 0;   // the next iteration's counter
  }
  km_offsets(a.total, a.k, s_seg, s_off);
  u64* st_count = a.status + ROVIT_KMEANS_WORDS;
  u64* st_medoid = st_count + a.k;
  double* st_inertia = reinterpret_cast<double*>(st_medoid + a.k);
  double* st_sil = st_inertia + a.k;
  double* st_radius = st_sil + a.k;
  for (int c = blockIdx.x; c < a.k; c += gridDim.x) {
    const int cnt = s_off[c + 1] - s_off[c], g0 = s_seg[c], g1 = s_seg[c + 1];
    if (a.stats) {
      if (tid == 0) {
        double in = 0.0, sl = 0.0;
        u64 key = EMPTY;
        unsigned rad = 0u;
        for (int g = g0; g < g1; ++g) {
          const u64* o = a.pst + (size_t)g * 4;
          in += __longlong_as_double((long long)o[0]);
          sl += __longlong_as_double((long long)o[1]);
          key = o[2] < key ? o[2] : key;
          rad = (unsigned)o[3] > rad ? (unsigned)o[3] : rad;
        }
        st_count[c] = (u64)cnt;
        st_medoid[c] = cnt > 0 ? (key & 0xffffffffull) : ~0ull;   // -1 as int64
        st_inertia[c] = in;
        st_sil[c] = sl;
        st_radius[c] = (double)__uint_as_float(rad);
        if (cnt == 0) atomicAdd(&a.status[ROVIT_KMEANS_EMPTY], 1ull);
      }
      continue;
    }
    if (cnt == 0) {                                              // keeps its centroid
      if (tid == 0) atomicAdd(&a.status[ROVIT_KMEANS_EMPTY_EVENTS], 1ull);
      continue;
    }
    double mean = 0.0;
    if (tid < a.E) {
      for (int g = g0; g < g1; ++g) mean += a.psum[(size_t)g * a.E + tid];
      mean /= (double)cnt;
    }
    __syncthreads();                                             // the previous cluster's LDS values have been read
    if (!a.cosine) {
      const float v = (float)mean;
      if (tid < a.E) {
        a.c[(size_t)c * a.E + tid] = v;
        s_c[tid] = v;
      }
      __syncthreads();
      if (tid == 0) {
        float s = 0.f;
        for (int f = 0; f < a.E; ++f) s = fmaf(s_c[f], s_c[f], s);
        a.cn[c] = s;
      }
    } else {
      s_m[tid] = mean;
      __syncthreads();
      double nn = 0.0;
      for (int f = 0; f < a.E; ++f) nn += s_m[f] * s_m[f];       // the same sum in every thread
      const bool good = nn > 0.0 && nn < __builtin_inf();
      if (good && tid < a.E) a.c[(size_t)c * a.E + tid] = (float)(mean / sqrt(nn));
      if (!good && tid == 0) atomicAdd(&a.status[ROVIT_KMEANS_ZERO_MEANS], 1ull);
    }
  }
  if (a.stats && blockIdx.x == 0 && tid == 0 && a.status[ROVIT_KMEANS_DONE] == 0) a.status[ROVIT_KMEANS_N_ITER] = (u64)a.max_iter;
}

// ---- contingency ------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NT) void km_contingency_kernel(const int* clusters, const int* classes, int n, int k, int C, u64* table) {
  const int chunks = (n + NT - 1) / NT;
  for (int w = blockIdx.x; w < chunks; w += gridDim.x) {
    const int row = w * NT + threadIdx.x;
    if (row < n) {
      const int c = clusters[row], y = classes[row];
      const bool in = c >= 0 && c < k && y >= 0 && y < C;
      atomicAdd(&table[in ? (size_t)c * C + y : (size_t)k * C], 1ull);
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------

int check_problem(const rovit_kmeans_problem* p, const char* who, int k, bool outputs) {
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_KMEANS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_KMEANS_MAX_ROWS);
  ROVIT_CHECK_ARG(p->embed >= 32 && p->embed <= 256 && p->embed % 32 == 0, ROVIT_ERR_SHAPE, "%s: embed %d (a multiple of 32 in 32..256)", who,
                  p->embed);
  ROVIT_CHECK_ARG(k >= 1 && k <= MAXK, ROVIT_ERR_SHAPE, "%s: %d clusters or seeds (1..%d)", who, k, MAXK);
  ROVIT_CHECK_ARG(p->metric == ROVIT_KNN_L2 || p->metric == ROVIT_KNN_COSINE, ROVIT_ERR_SHAPE, "%s: metric %d", who, p->metric);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->features && p->centroids && p->workspace && p->status, ROVIT_ERR_NULL, "%s: a null pointer", who);
  ROVIT_CHECK_ARG((p->metric == ROVIT_KNN_COSINE) == (p->normalized != nullptr), ROVIT_ERR_NULL,
                  "%s: the normalized scratch goes with the cosine metric and with no other", who);
  ROVIT_CHECK_ARG(!outputs || (p->labels && p->distance && p->second_distance && p->silhouette), ROVIT_ERR_NULL,
                  "%s: an output is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->features) && rovit_aligned16(p->normalized) && rovit_aligned16(p->centroids) && rovit_aligned16(p->workspace),
                  ROVIT_ERR_ALIGN, "%s: the rows, the centroids or the workspace are not 16-byte aligned", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->seeds, 4) && rovit_aligned(p->tap, 4) && rovit_aligned(p->labels, 4) && rovit_aligned(p->distance, 4) &&
                      rovit_aligned(p->second_distance, 4) && rovit_aligned(p->silhouette, 4) && rovit_aligned(p->status, 8),
                  ROVIT_ERR_ALIGN, "%s: an array is not aligned to its element size", who);
  const size_t need = layout_of(p->n, p->embed, k).bytes;
  ROVIT_CHECK_ARG(p->workspace_bytes >= need, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes, need);
  return ROVIT_OK;
}

struct Ctx {
  const rovit_kmeans_problem* p;
  Layout l;
  char* ws;
  hipStream_t s;
  bool cosine;
  const float* rows;
  dim3 grid(long long items) const { return rovit_grid(items, p->max_workgroups); }
};

inline Ctx ctx_of(const rovit_kmeans_problem* p, int k, rovit_stream_t stream) {
  Ctx c;
  c.p = p;
  c.l = layout_of(p->n, p->embed, k);
  c.ws = (char*)p->workspace;
  c.s = (hipStream_t)stream;
  c.cosine = p->metric == ROVIT_KNN_COSINE;
  c.rows = c.cosine ? p->normalized : p->features;
  return c;
}

int launch_rows(const Ctx& c, size_t status_words, const char* who) {
  if (hipMemsetAsync(c.p->status, 0, status_words * 8, c.s) != hipSuccess || hipMemsetAsync(c.ws + c.l.scal, 0, S_WORDS * 8, c.s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  RowArgs a;
  a.n = c.p->n; a.E = c.p->embed; a.cosine = c.cosine;
  a.x = c.p->features; a.norm = (float*)(c.ws + c.l.norm); a.ok = (int*)(c.ws + c.l.ok); a.xhat = c.p->normalized; a.status = (u64*)c.p->status;
  hipLaunchKernelGGL(km_rows_kernel, c.grid(c.l.nb), dim3(NT), 0, c.s, a);
  ROVIT_CHECK_LAUNCH("km_rows_kernel");
  return ROVIT_OK;
}

int launch_assign(const Ctx& c, int force, int it, const char* who) {
  const rovit_kmeans_problem* p = c.p;
  AssignArgs a;
  a.n = p->n; a.E = p->embed; a.k = p->k; a.cosine = c.cosine; a.force = force; a.parity = it & 1;
  a.x = c.rows; a.xn = (const float*)(c.ws + c.l.norm); a.ok = (const int*)(c.ws + c.l.ok);
  a.c = p->centroids; a.cn = (const float*)(c.ws + c.l.cnorm);
  a.labels = p->labels; a.d1 = p->distance; a.d2 = p->second_distance; a.sil = p->silhouette; a.status = (u64*)p->status;
  const size_t lds = assign_lds_bytes(p->embed);
  ROVIT_CHECK_ARG(rovit_set_max_lds((const void*)km_assign_kernel, lds), ROVIT_ERR_LAUNCH, "%s: cannot raise the LDS limit", who);
  const long long tiles = ((long long)p->n + QT - 1) / QT;        // two workgroups per CU walk the tiles: the next tile's loads fly behind the products
  hipLaunchKernelGGL(km_assign_kernel, c.grid(tiles < ASSIGN_WGS ? tiles : ASSIGN_WGS), dim3(NT), lds, c.s, a);
  ROVIT_CHECK_LAUNCH("km_assign_kernel");
  return ROVIT_OK;
}

// the sort by label, the segment sums and the finalize launch of iteration `it` (stats: the final pass)
int launch_update(const Ctx& c, int force, int it, int stats) {
  const rovit_kmeans_problem* p = c.p;
  SortArgs sa;
  sa.n = p->n; sa.k = p->k; sa.it = it; sa.force = force;
  sa.labels = p->labels; sa.cnt = (int*)(c.ws + c.l.cnt); sa.base = (int*)(c.ws + c.l.base); sa.total = (int*)(c.ws + c.l.total);
  sa.order = (int*)(c.ws + c.l.order); sa.status = (const u64*)p->status;
  hipLaunchKernelGGL(km_count_kernel, c.grid(c.l.nb), dim3(NT), 0, c.s, sa);
  ROVIT_CHECK_LAUNCH("km_count_kernel");
  hipLaunchKernelGGL(km_scan_kernel, c.grid(p->k), dim3(NT), 0, c.s, sa);
  ROVIT_CHECK_LAUNCH("km_scan_kernel");
  hipLaunchKernelGGL(km_scatter_kernel, c.grid(c.l.nb), dim3(NT), 0, c.s, sa);
  ROVIT_CHECK_LAUNCH("km_scatter_kernel");
  UpdArgs ua;
  ua.n = p->n; ua.E = p->embed; ua.k = p->k; ua.cosine = c.cosine; ua.it = it; ua.force = force; ua.stats = stats; ua.max_iter = p->max_iter;
  ua.x = c.rows; ua.order = sa.order; ua.total = sa.total; ua.d1 = p->distance; ua.sil = p->silhouette;
  ua.psum = (double*)(c.ws + c.l.psum); ua.pst = (u64*)(c.ws + c.l.pst); ua.c = p->centroids; ua.cn = (float*)(c.ws + c.l.cnorm);
  ua.status = (u64*)p->status;
  hipLaunchKernelGGL(km_partial_kernel, c.grid(c.l.nseg), dim3(NT), 0, c.s, ua);
  ROVIT_CHECK_LAUNCH("km_partial_kernel");
  hipLaunchKernelGGL(km_finalize_kernel, c.grid(p->k), dim3(NT), 0, c.s, ua);
  ROVIT_CHECK_LAUNCH("km_finalize_kernel");
  return ROVIT_OK;
}

}  // namespace

extern "C" size_t rovit_kmeans_workspace_bytes(int n, int embed, int k) { return limits_ok(n, embed, k) ? layout_of(n, embed, k).bytes : 0; }

extern "C" int rovit_kmeans_seed(const rovit_kmeans_problem* p, rovit_stream_t stream) {
  const char* who = "kmeans_seed";
  if (int rc = check_problem(p, who, p ? p->m : 0, false)) return rc;
  ROVIT_CHECK_ARG(p->seeds, ROVIT_ERR_NULL, "%s: seeds is a null pointer", who);
  ROVIT_CHECK_ARG(p->restart >= 0, ROVIT_ERR_SHAPE, "%s: restart %d (>= 0)", who, p->restart);
  const Ctx c = ctx_of(p, p->m, stream);
  if (int rc = launch_rows(c, ROVIT_KMEANS_WORDS, who)) return rc;
  SeedArgs a;
  a.n = p->n; a.E = p->embed; a.cosine = c.cosine; a.restart = p->restart; a.seed = p->seed;
  a.x = c.rows; a.norm = (const float*)(c.ws + c.l.norm); a.ok = (const int*)(c.ws + c.l.ok); a.mind = (float*)(c.ws + c.l.mind);
  a.blockw = (u64*)(c.ws + c.l.blockw); a.blockv = (u64*)(c.ws + c.l.blockv); a.dmax = (unsigned*)(c.ws + c.l.scal + S_DMAX * 8);
  a.seeds = p->seeds; a.centroids = p->centroids; a.cnorm = (float*)(c.ws + c.l.cnorm); a.tap = p->tap; a.status = (u64*)p->status;
  for (int j = 0; j < p->m; ++j) {
    a.j = j;
    if (j > 0) {
      hipLaunchKernelGGL(km_seed_dist_kernel, c.grid(c.l.nb), dim3(NT), 0, c.s, a);
      ROVIT_CHECK_LAUNCH("km_seed_dist_kernel");
    }
    hipLaunchKernelGGL(km_seed_weights_kernel, c.grid(c.l.nb), dim3(NT), 0, c.s, a);
    ROVIT_CHECK_LAUNCH("km_seed_weights_kernel");
    hipLaunchKernelGGL(km_seed_pick_kernel, dim3(1), dim3(NT), 0, c.s, a);
    ROVIT_CHECK_LAUNCH("km_seed_pick_kernel");
  }
  return ROVIT_OK;
}

extern "C" int rovit_kmeans_run(const rovit_kmeans_problem* p, rovit_stream_t stream) {
  const char* who = "kmeans_run";
  if (int rc = check_problem(p, who, p ? p->k : 0, true)) return rc;
  ROVIT_CHECK_ARG(p->max_iter >= 1 && p->max_iter <= ROVIT_KMEANS_MAX_ITER, ROVIT_ERR_SHAPE, "%s: max_iter %d (1..%d)", who, p->max_iter,
                  ROVIT_KMEANS_MAX_ITER);
  const Ctx c = ctx_of(p, p->k, stream);
  if (int rc = launch_rows(c, ROVIT_KMEANS_WORDS + 5 * (size_t)p->k, who)) return rc;
  if (hipMemsetAsync(p->labels, 0xff, (size_t)p->n * 4, c.s) != hipSuccess) {   // -1: every valid row changes in iteration 1
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(km_cnorm_kernel, dim3((p->k + NT - 1) / NT), dim3(NT), 0, c.s, (const float*)p->centroids, (float*)(c.ws + c.l.cnorm), p->k,
                     p->embed);
  ROVIT_CHECK_LAUNCH("km_cnorm_kernel");
  for (int it = 1; it <= p->max_iter; ++it) {
    if (int rc = launch_assign(c, 0, it, who)) return rc;
    if (int rc = launch_update(c, 0, it, 0)) return rc;
  }
  if (int rc = launch_assign(c, 1, 0, who)) return rc;
  return launch_update(c, 1, 0, 1);
}

extern "C" int rovit_kmeans_assign(const rovit_kmeans_problem* p, rovit_stream_t stream) {
  const char* who = "kmeans_assign";
  if (int rc = check_problem(p, who, p ? p->k : 0, true)) return rc;
  const Ctx c = ctx_of(p, p->k, stream);
  if (int rc = launch_rows(c, ROVIT_KMEANS_WORDS, who)) return rc;
  hipLaunchKernelGGL(km_cnorm_kernel, dim3((p->k + NT - 1) / NT), dim3(NT), 0, c.s, (const float*)p->centroids, (float*)(c.ws + c.l.cnorm), p->k,
                     p->embed);
  ROVIT_CHECK_LAUNCH("km_cnorm_kernel");
  return launch_assign(c, 1, 0, who);
}

extern "C" int rovit_kmeans_contingency(const int* clusters, const int* classes, int n, int k, int num_classes, long long* table,
                                        rovit_stream_t stream) {
  const char* who = "kmeans_contingency";
  ROVIT_CHECK_ARG(clusters && classes && table, ROVIT_ERR_NULL, "%s: a null pointer", who);
  ROVIT_CHECK_ARG(n >= 1 && n <= ROVIT_KMEANS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, n, ROVIT_KMEANS_MAX_ROWS);
  ROVIT_CHECK_ARG(k >= 1 && k <= MAXK, ROVIT_ERR_SHAPE, "%s: %d clusters (1..%d)", who, k, MAXK);
  ROVIT_CHECK_ARG(num_classes >= 1 && num_classes <= ROVIT_KNN_MAX_CLASSES, ROVIT_ERR_SHAPE, "%s: %d classes (1..%d)", who, num_classes,
                  ROVIT_KNN_MAX_CLASSES);
  ROVIT_CHECK_ARG(rovit_aligned(clusters, 4) && rovit_aligned(classes, 4) && rovit_aligned(table, 8), ROVIT_ERR_ALIGN,
                  "%s: an array is not aligned to its element size", who);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(table, 0, ((size_t)k * num_classes + 1) * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(km_contingency_kernel, dim3((n + NT - 1) / NT), dim3(NT), 0, s, clusters, classes, n, k, num_classes, (u64*)table);
  ROVIT_CHECK_LAUNCH("km_contingency_kernel");
  return ROVIT_OK;
}
