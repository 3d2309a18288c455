// Training-data influence through the last layer of a head on the device: the whitened last-layer gradients of feature rows
// (rovit_influence_embed) and the signed top-k inner-product search over them (rovit_influence_search).  Koh & Liang, ICML 2017; Pruthi
// et al., NeurIPS 2020; Barshan et al., AISTATS 2020.  The reference has no counterpart.  Definitions, sign and scale: include/rovit_hip.h.
//
// With W = R^-1 of the Laplace posterior precision H + tau I = R R^T and the last-layer gradient g = r (x) a of a row, u = W g is its
// whitened gradient and g_t^T (H + tau I)^-1 g_j = u_t . u_j: influence is a dot product, self-influence a squared norm.
//
//   inf_embed_kernel   a workgroup owns 64 rows.  Prologue: the feature rows into LDS (laplace_device.h), a wave per row looks for a
//                      non-finite feature, then a thread per row forms the residual r in fp64 (rounded once) and the row's status.  The
//                      hidden rows are formed in LDS by lap_hidden and W is streamed exactly as lap_predict_kernel streams it: per class
//                      block cb and pair of its 32-row tiles, per class block c <= cb the tile's columns of block c (up to the diagonal
//                      tile for c = cb), z_c on the exact-fp32 matrix instruction, one row per lane.  Epilogue of an output tile:
//                      u = sum_{c <= cb} r_c z_c, one fma chain in ascending c, stored as four float4 per lane; |u|^2 is accumulated
//                      in fp64 per lane in tile order, the four partials of a row (two lane halves, two wave pairs) are added in a fixed
//                      order and rounded once.  (The strictly ascending chain differs from this order by a few units of 2^-53, far
//                      below the one rounding to fp32.)  A non-finite entry of u makes the norm non-finite: the row is then zeroed again.
//   inf_search_kernel  a work item = (query tile of 64 rows, reference split).  A 64 x 640 fp32 query tile is the whole LDS of a CU, so the
//                      dim is walked in slabs of 64 columns: the query slab and the slab of one 64-row reference tile sit in LDS in the
//                      (f0 f2 f4 f6 | f1 f3 f5 f7) order of store_unit (feature_tiles.h), the next slab's loads are in flight in registers while this
//                      slab's products run, and wave (qt, rt) keeps ONE accumulator tile over all slabs of a reference tile: a k-ordered
//                      fp32 fma chain per (query, row), the queries on the lane index.  BOTH ends are kept in one pass: a lane has two
//                      ascending key lists of KB keys in registers, proponents under the key (~o << 32) | j and opponents under
//                      (o << 32) | j, o the orderable bits of the score with -0 made +0.  The four lists of a query and end meet in LDS,
//                      are ranked by merge_four (topk_device.h), and the KB smallest go to the workspace (B, 2, splits, KB).
//   inf_merge_kernel   a wave per (query, end): the splits' lists to LDS, every key with a position below k ranked by binary searches
//                      in the other lists, the k smallest decoded; labels and severities gathered.
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), VGPRs + AGPRs: inf_search_kernel<32> 231 + 16 with both ends in
// one pass, <16> 216 + 16, <8> 135 + 16; inf_embed_kernel 241 + 16; inf_merge_kernel 24.  ScratchSize is 0 for every kernel of this file.
// Work items are walked with a stride of the grid; no floating-point atomic; no result depends on which workgroup computes it, on the
// number of reference splits, or on how the rows were split into embed calls (a row's outputs are a function of that row alone).
#include "common.h"
#include "feature_tiles.h"
#include "laplace_device.h"
#include "topk_device.h"

namespace {

using namespace ftile;                           // tile_dot, acc_row, store_unit
using namespace laplace;                         // NT, MAXC, ROWS, lap_hidden, lap_stage_features
using namespace topk;                            // u64, EMPTY, key_of, keys_below, list_insert, merge_four, Plan, plan_of

// ---- embed -----------------------------------------------------------------------------------------------------------------------------

enum { ST_OK = 0, ST_BAD_ROW = 1, ST_BAD_LABEL = 2, ST_OUTSIDE = 3, ST_ZERO = 4 };

// As [64][SA], the region of the feature rows and the W tiles, the norm partials [64][4] (doubles), the residuals [64][MAXC], the row
// flags [64], the status [64], the rows to zero again [64]
inline size_t embed_lds_bytes(int E, int hid) {
  return ((size_t)ROWS * (hid + 36) + lap_stream_region(E, hid) + ROWS * 8 + ROWS * MAXC + 3 * ROWS) * 4;
}

__global__ __launch_bounds__(NT) void inf_embed_kernel(const rovit_influence_rows a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int E = a.embed, hid = a.hid, C = a.num_classes, n = a.n, P = hid + 32, SA = hid + 36, TP = P / 32, P4 = P / 4;
  const int N = C * P;                                          // W is (N, N), a row of u is N wide
  float* As = lds;                                              // [64][SA] augmented hidden rows
  float* Fs = As + ROWS * SA;                                   // [64][E + 4] feature rows, then
  float* Ws = Fs;                                               // [2][32][SA] one tile of W per wave pair
  double* s_nrm = reinterpret_cast<double*>(Fs + lap_stream_region(E, hid));   // [64][4]
  float* s_r = reinterpret_cast<float*>(s_nrm + ROWS * 4);      // [64][MAXC]
  int* s_ok = reinterpret_cast<int*>(s_r + ROWS * MAXC);        // [64]
  int* s_st = s_ok + ROWS;                                      // [64]
  int* s_again = s_st + ROWS;                                   // [64]
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), rt = wv & 1, th = wv >> 1;
  const int tiles = (n + ROWS - 1) / ROWS;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = tile * ROWS;
    __syncthreads();
    lap_stage_features(Fs, a.features, r0, n, E);
    for (int rr = 0; rr < 16; ++rr) {                           // a wave per row: is any feature non-finite?
      const int lr = wv * 16 + rr, row = r0 + lr;
      bool bad = false;
      if (row < n)
        for (int e = lane; e < E; e += 64) bad |= !isfinite(a.features[(size_t)row * E + e]);
      const bool any_bad = __ballot(bad) != 0ull;
      if (lane == 0) s_ok[lr] = (row < n && !any_bad) ? 1 : 0;
    }
    __syncthreads();
    if (tid < ROWS) {                                           // a thread per row: the residual in fp64, rounded once, and the status
      const int row = r0 + tid;
      int st = row < n ? (s_ok[tid] ? ST_OK : ST_BAD_ROW) : ST_OUTSIDE;
      float r[MAXC];
#pragma unroll
      for (int c = 0; c < MAXC; ++c) r[c] = 0.f;
      if (st == ST_OK && a.head == ROVIT_INFLUENCE_CLS) {
        const float* lg = a.cls_logits + (size_t)row * C;
        double e[MAXC];
        double m = 0.0;
        int am = 0;
        bool fin = true;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) {
            const float l = lg[c];
            fin &= isfinite(l);
            e[c] = (double)l;
            if (c == 0 || e[c] > m) { m = e[c]; am = c; }
          }
        const int y = a.labels ? a.labels[row] : am;
        if (!fin) st = ST_BAD_ROW;
        else if (y < 0 || y >= C) st = ST_BAD_LABEL;
        else if (a.target == ROVIT_INFLUENCE_LOSS) {
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < MAXC; ++c)
            if (c < C) {
              e[c] = exp(e[c] - m);
              s += e[c];
            }
#pragma unroll
          for (int c = 0; c < MAXC; ++c)
            if (c < C) r[c] = (float)(e[c] / s - (c == y ? 1.0 : 0.0));
        } else {
#pragma unroll
          for (int c = 0; c < MAXC; ++c) r[c] = c == y ? 1.f : 0.f;
        }
      } else if (st == ST_OK) {                                 // the Gaussian head: C = 1
        if (a.target == ROVIT_INFLUENCE_LOSS) {
          const float mu = a.mu[row], lv = a.log_var[row], sv = a.severity[row];
          const double w = exp(-(double)lv);
          r[0] = (float)(((double)mu - (double)sv) * w);
          if (!(isfinite(mu) && isfinite(lv) && isfinite(sv) && isfinite((float)w) && isfinite(r[0]))) st = ST_BAD_ROW;
        } else {
          r[0] = 1.f;
        }
      }
      s_ok[tid] = st == ST_OK ? 1 : 0;
      s_st[tid] = st;
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        s_r[tid * MAXC + c] = st == ST_OK ? r[c] : 0.f;
        if (c < C && row < n) a.residual[(size_t)row * C + c] = st == ST_OK ? r[c] : __builtin_nanf("");
      }
    }
    __syncthreads();
    lap_hidden(Fs, As, s_ok, a.fc1_weight, a.fc1_bias, E, hid);
    float res[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) res[c] = s_r[(rt * 32 + l31) * MAXC + c];
    double nrm = 0.0;
    const int row = r0 + rt * 32 + l31;                         // this lane's row
    const float* frow = As + (rt * 32 + l31) * SA + 4 * lh;     // B[k][n = row]
    const float* wrow = Ws + (th * 32 + l31) * SA + 4 * lh;     // A[m = t][k]: plain rows, lane half h holds k = kk + 4 h + s in step s
    for (int cb = 0; cb < C; ++cb) {
      for (int at0 = 0; at0 < TP; at0 += 2) {
        const int at = at0 + th;                                // this wave's tile of class block cb
        const bool live = at < TP;
        f32x16 acc[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c <= cb) {                                        // uniform over the workgroup
            __syncthreads();                                    // the first one also closes lap_hidden's writes and Fs' reads
            for (int idx = tid; idx < 64 * P4; idx += NT) {     // rows of tiles at0, at0 + 1 of block cb, columns of block c
              const int wr = idx / P4, c4 = idx - wr * P4, t2 = at0 + (wr >> 5);
              const int kend2 = c == cb ? 32 * t2 + 32 : P;
              if (t2 < TP && 4 * c4 < kend2)
                *reinterpret_cast<float4*>(Ws + wr * SA + 4 * c4) =
                    *reinterpret_cast<const float4*>(a.whitening + (size_t)(cb * P + 32 * t2 + (wr & 31)) * N + (size_t)c * P + 4 * c4);
            }
            __syncthreads();
            if (live) {
              const int kend = c == cb ? 32 * at + 32 : P;
              acc[c] = tile_dot(acc[c], wrow, frow, kend);
            }
          }
        // lane (l31, h) holds z_c[row l31][t = 32 at + acc_row(r, h)] of every c <= cb
        if (live) {
          float u[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) u[r] = 0.f;
#pragma unroll
          for (int c = 0; c < MAXC; ++c)
            if (c <= cb) {
#pragma unroll
              for (int r = 0; r < 16; ++r) u[r] = fmaf(res[c], acc[c][r], u[r]);
            }
#pragma unroll
          for (int r = 0; r < 16; ++r) nrm = fma((double)u[r], (double)u[r], nrm);
          if (row < n) {
            float* out = a.rows + (size_t)row * N + (size_t)cb * P + 32 * at + 4 * lh;
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<float4*>(out + 8 * g) = make_float4(u[4 * g], u[4 * g + 1], u[4 * g + 2], u[4 * g + 3]);
          }
        }
      }
    }
    s_nrm[(rt * 32 + l31) * 4 + th * 2 + lh] = nrm;
    __syncthreads();
    if (tid < ROWS) {                                           // wave 0: the norm, the final status, the counts
      const int grow = r0 + tid;
      const double total = ((s_nrm[tid * 4] + s_nrm[tid * 4 + 1]) + s_nrm[tid * 4 + 2]) + s_nrm[tid * 4 + 3];
      const float f = (float)total;
      int st = s_st[tid];
      bool again = false;
      if (st == ST_OK) {
        if (!isfinite(f)) { st = ST_BAD_ROW; again = true; }
        else if (total == 0.0) st = ST_ZERO;
      }
      s_again[tid] = again ? 1 : 0;
      if (grow < n) {
        a.norm2[grow] = st == ST_OK ? f : 0.f;
        a.valid[grow] = st == ST_OK ? 1 : 0;
      }
      const unsigned long long in = __popcll(__ballot(st != ST_OUTSIDE)), good = __popcll(__ballot(st == ST_OK)),
                               bad = __popcll(__ballot(st == ST_BAD_ROW)), lab = __popcll(__ballot(st == ST_BAD_LABEL));
      if (tid == 0) {
        unsigned long long* cnt = (unsigned long long*)a.counts;
        atomicAdd(&cnt[ROVIT_INFLUENCE_N], in);
        if (good) atomicAdd(&cnt[ROVIT_INFLUENCE_N_VALID], good);
        if (bad) atomicAdd(&cnt[ROVIT_INFLUENCE_BAD_ROWS], bad);
        if (lab) atomicAdd(&cnt[ROVIT_INFLUENCE_BAD_LABELS], lab);
      }
    }
    __syncthreads();
    for (int lr = 0; lr < ROWS; ++lr)                           // a row with a non-finite entry is stored as zeros, like every invalid row
      if (s_again[lr] != 0)
        for (int idx = tid; idx < N / 4; idx += NT)
          *reinterpret_cast<float4*>(a.rows + (size_t)(r0 + lr) * N + 4 * idx) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// ---- search ----------------------------------------------------------------------------------------------------------------------------

constexpr int QT = 64;                           // query rows of a work item
constexpr int RT = 64;                           // reference rows of an LDS tile
constexpr int KS = 64;                           // columns of a slab
constexpr int SST = KS + 4;                      // row stride of a slab in LDS
constexpr int MAXK = ROVIT_INFLUENCE_MAX_K;
constexpr int UNITS = (QT + RT) * (KS / 8) / NT; // units of 8 columns a thread moves per slab
static_assert(QT == 64 && RT == 64 && UNITS == 4, "2 x 2 sub-tiles of 32 per workgroup, one per wave; plan_of's tiles");

inline bool search_limits_ok(int B, int n, int dim, int k) {
  return B >= 1 && n >= 1 && n <= ROVIT_KAN_STATS_MAX_ROWS && dim >= 32 && dim <= ROVIT_INFLUENCE_MAX_DIM && dim % 32 == 0 && k >= 1 && k <= MAXK;
}

inline size_t keys_bytes(int B, const Plan& p) { return rovit_up16((size_t)B * 2 * p.splits * p.kb * 8); }

struct SearchArgs {
  int B, n, dim, relative, qtiles, rtiles, splits, tps;
  const float* q;
  const int* qok;           // or nullptr
  const float* r;
  const float* rnorm;
  const int* rok;
  const int* exclude;       // or nullptr
  u64* keys;                // (B, 2, splits, KB)
};

inline size_t search_lds_bytes(int kb) {
  const size_t stage = ((size_t)(QT + RT) * SST + 2 * RT) * 4, merge = (size_t)QT * 4 * kb * 8;
  return stage > merge ? stage : merge;
}

template <int KB>
__global__ __launch_bounds__(NT) void inf_search_kernel(const SearchArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dim = a.dim, nslab = (dim + KS - 1) / KS;
  float* Qs = lds;                                               // [64][SST] the query slab
  float* Rs = Qs + QT * SST;                                     // [64][SST] the slab of one reference tile
  float* s_rl = Rs + RT * SST;                                   // [64] the divisor of the tile's rows: |u_j|, or 1
  int* s_rj = reinterpret_cast<int*>(s_rl + RT);                 // [64] their indices, -1: not a candidate
  u64* Ms = reinterpret_cast<u64*>(lds);                         // [64][4][KB] the lists of a tile's queries, over the staging buffers
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), qtw = wv >> 1, rtw = wv & 1;
  const int items = a.qtiles * a.splits;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int qt = item % a.qtiles, sp = item / a.qtiles, q0 = qt * QT;
    const int qrow = q0 + qtw * 32 + l31;
    const bool qgood = qrow < a.B && (!a.qok || a.qok[qrow] != 0);
    const int excl = (qgood && a.exclude) ? a.exclude[qrow] : -1;
    u64 pro[KB], opp[KB];
#pragma unroll
    for (int i = 0; i < KB; ++i) pro[i] = opp[i] = EMPTY;
    const int t0 = sp * a.tps, t1 = min(a.rtiles, t0 + a.tps), steps = (t1 - t0) * nslab;
    float4 pu[UNITS], pv[UNITS];
    float p_rl = 1.f;
    int p_rj = -1;
    auto fetch = [&](int t, int s) {                             // slab s of the queries and of tile t into registers; rows that do not count become zeros
#pragma unroll
      for (int i = 0; i < UNITS; ++i) {
        const int idx = tid + NT * i, row = idx >> 3, col = s * KS + 8 * (idx & 7);
        pu[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        pv[i] = pu[i];
        const float* src = nullptr;
        if (col < dim) {
          if (row < QT) {
            const int g = q0 + row;
            if (g < a.B && (!a.qok || a.qok[g] != 0)) src = a.q + (size_t)g * dim + col;
          } else {
            const int j = t * RT + row - QT;
            if (j < a.n && a.rok[j] != 0) src = a.r + (size_t)j * dim + col;
          }
        }
        if (src) {
          pu[i] = reinterpret_cast<const float4*>(src)[0];
          pv[i] = reinterpret_cast<const float4*>(src)[1];
        }
      }
      if (s == 0 && tid < RT) {
        const int j = t * RT + tid;
        const bool ok = j < a.n && a.rok[j] != 0 && (!a.relative || a.rnorm[j] > 0.f);
        p_rl = (ok && a.relative) ? sqrtf(a.rnorm[j]) : 1.f;
        p_rj = ok ? j : -1;
      }
    };
    if (steps > 0) fetch(t0, 0);
    f32x16 acc;
    int t = t0, s = 0;
    for (int it = 0; it < steps; ++it) {
      __syncthreads();                                           // the previous slab's products are done, and the previous item's lists read
#pragma unroll
      for (int i = 0; i < UNITS; ++i) {
        const int idx = tid + NT * i, row = idx >> 3, c8 = idx & 7;
        store_unit((row < QT ? Qs + row * SST : Rs + (row - QT) * SST) + 8 * c8, pu[i], pv[i]);
      }
      if (s == 0 && tid < RT) {
        s_rl[tid] = p_rl;
        s_rj[tid] = p_rj;
      }
      __syncthreads();
      const int sn = s + 1 < nslab ? s + 1 : 0, tn = sn ? t : t + 1;
      if (it + 1 < steps) fetch(tn, sn);                         // in flight behind the products below
      if (s == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      }
      const float* rrow = Rs + (rtw * 32 + l31) * SST + 4 * lh;  // A[m = reference][k]: lane half h holds column 8 b + 2 s + h in step s
      const float* qrw = Qs + (qtw * 32 + l31) * SST + 4 * lh;   // B[k][n = query]
      acc = tile_dot(acc, rrow, qrw, KS);                             // a compile-time bound: unrolled
      if (sn == 0) {
        // lane (l31, h) holds q.r of query l31 against the sub-tile's rows acc_row(r, h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = rtw * 32 + acc_row(r, lh);
          const int j = s_rj[i];
          const float sc = (a.relative ? acc[r] / s_rl[i] : acc[r]) + 0.f;       // -0 becomes +0
          const bool cand = qgood && j >= 0 && j != excl && isfinite(sc);
          const unsigned b = __float_as_uint(sc), o = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);   // ascending as unsigned
          const u64 kp = cand ? key_of(~o, j) : EMPTY;
          const u64 ko = cand ? key_of(o, j) : EMPTY;
          if (__ballot(kp < pro[KB - 1]) != 0ull) list_insert<KB>(pro, kp);
          if (__ballot(ko < opp[KB - 1]) != 0ull) list_insert<KB>(opp, ko);
        }
      }
      s = sn;
      t = tn;
    }
    const int slot = (qtw * 32 + l31) * 4 + rtw * 2 + lh, g = q0 + (tid >> 2);   // g: the query whose lists this thread helps to merge
    u64* out = g < a.B ? a.keys + ((size_t)g * 2 * a.splits + sp) * KB : nullptr;  // (B, 2, splits, KB): the proponents' words
    merge_four<KB>(pro, Ms, slot, out);
    merge_four<KB>(opp, Ms, slot, out ? out + (size_t)a.splits * KB : nullptr);
  }
}

inline size_t merge_lds_bytes(int splits, int kb) { return ((size_t)splits * kb + MAXK) * 8; }

__global__ __launch_bounds__(64) void inf_merge_kernel(const rovit_influence_query a, const u64* keys, int splits, int KB) {
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  u64* L = sm;                                                   // [splits][KB]
  u64* top = L + splits * KB;                                    // [MAXK]
  const int lane = threadIdx.x, k = a.k, total = splits * KB;
  const long long items = 2ll * a.batch;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const int q = (int)(w >> 1), end = (int)(w & 1);
    __syncthreads();
    for (int i = lane; i < total; i += 64) L[i] = keys[(size_t)w * total + i];
    if (lane < MAXK) top[lane] = EMPTY;
    __syncthreads();
    // real keys are distinct (the index is part of the key): a key's rank is its position in its own list plus the keys below it in the
    // others; a key at position k or beyond in its own list cannot be among the k smallest
    for (int i = lane; i < total; i += 64) {
      const int s = i / KB, p = i - s * KB;
      const u64 c = L[i];
      if (c == EMPTY || p >= k) continue;
      int rank = p;
      for (int l = 0; l < splits && rank < k; ++l)
        if (l != s) rank += keys_below(L + l * KB, KB, c);
      if (rank < k) top[rank] = c;
    }
    __syncthreads();
    if (lane < k) {
      const u64 c = top[lane];
      const bool real = c != EMPTY;
      const int j = real ? key_index(c) : -1;
      const unsigned hi = key_bits(c), o = end == 0 ? ~hi : hi, b = o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu);
      const float sc = real ? __uint_as_float(b) : __builtin_nanf("");
      const size_t at = (size_t)q * k + lane;
      (end == 0 ? a.pro_scores : a.opp_scores)[at] = sc;
      (end == 0 ? a.pro_indices : a.opp_indices)[at] = j;
      if (a.ref_labels) (end == 0 ? a.pro_labels : a.opp_labels)[at] = real ? a.ref_labels[j] : -1;
      if (a.ref_severity) (end == 0 ? a.pro_severities : a.opp_severities)[at] = real ? a.ref_severity[j] : __builtin_nanf("");
    }
  }
}

template <int KB>
bool launch_search(dim3 grid, size_t lds, hipStream_t s, const SearchArgs& a) {
  if (!rovit_set_max_lds((const void*)inf_search_kernel<KB>, lds)) return false;
  hipLaunchKernelGGL(inf_search_kernel<KB>, grid, dim3(NT), lds, s, a);
  return true;
}

}  // namespace

extern "C" int rovit_influence_embed(const rovit_influence_rows* p, rovit_stream_t stream) {
  const char* who = "influence_embed";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_KAN_STATS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_KAN_STATS_MAX_ROWS);
  ROVIT_CHECK_ARG(p->embed >= 32 && p->embed <= 256 && p->embed % 32 == 0, ROVIT_ERR_SHAPE, "%s: embed %d (a multiple of 32 in 32..256)", who,
                  p->embed);
  ROVIT_CHECK_ARG(p->hid >= 32 && p->hid <= 256 && p->hid % 32 == 0, ROVIT_ERR_SHAPE, "%s: hid %d (a multiple of 32 in 32..256)", who, p->hid);
  ROVIT_CHECK_ARG(p->num_classes >= 1 && p->num_classes <= MAXC, ROVIT_ERR_SHAPE, "%s: %d classes (1..%d)", who, p->num_classes, MAXC);
  ROVIT_CHECK_ARG(p->head == ROVIT_INFLUENCE_CLS || p->head == ROVIT_INFLUENCE_MU, ROVIT_ERR_SHAPE, "%s: head %d", who, p->head);
  ROVIT_CHECK_ARG(p->target == ROVIT_INFLUENCE_LOSS || p->target == ROVIT_INFLUENCE_OUTPUT, ROVIT_ERR_SHAPE, "%s: target %d", who, p->target);
  ROVIT_CHECK_ARG(p->head != ROVIT_INFLUENCE_MU || p->num_classes == 1, ROVIT_ERR_SHAPE, "%s: the Gaussian head has one output, got %d", who,
                  p->num_classes);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->features && p->fc1_weight && p->fc1_bias && p->whitening, ROVIT_ERR_NULL,
                  "%s: the features, fc1 or the whitening table are missing (null pointer)", who);
  ROVIT_CHECK_ARG(p->head != ROVIT_INFLUENCE_CLS || p->cls_logits, ROVIT_ERR_NULL, "%s: the classification head needs cls_logits", who);
  ROVIT_CHECK_ARG(p->head != ROVIT_INFLUENCE_MU || p->target != ROVIT_INFLUENCE_LOSS || (p->mu && p->log_var && p->severity), ROVIT_ERR_NULL,
                  "%s: the Gaussian head's loss needs mu, log_var and severity", who);
  ROVIT_CHECK_ARG(p->rows && p->residual && p->norm2 && p->valid && p->counts, ROVIT_ERR_NULL, "%s: an output is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->features) && rovit_aligned16(p->fc1_weight) && rovit_aligned16(p->whitening) && rovit_aligned16(p->rows),
                  ROVIT_ERR_ALIGN, "%s: the features, fc1_weight, the whitening matrix or the rows are not 16-byte aligned", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->fc1_bias, 4) && rovit_aligned(p->cls_logits, 4) && rovit_aligned(p->labels, 4) && rovit_aligned(p->mu, 4) &&
                      rovit_aligned(p->log_var, 4) && rovit_aligned(p->severity, 4) && rovit_aligned(p->residual, 4) &&
                      rovit_aligned(p->norm2, 4) && rovit_aligned(p->valid, 4) && rovit_aligned(p->counts, 8),
                  ROVIT_ERR_ALIGN, "%s: an array is not aligned to its element size", who);
  const size_t lds = embed_lds_bytes(p->embed, p->hid);
  ROVIT_CHECK_ARG(rovit_set_max_lds((const void*)inf_embed_kernel, lds), ROVIT_ERR_LAUNCH, "%s: cannot raise the LDS limit", who);
  hipLaunchKernelGGL(inf_embed_kernel, rovit_grid(((long long)p->n + ROWS - 1) / ROWS, p->max_workgroups), dim3(NT), lds, (hipStream_t)stream, *p);
  ROVIT_CHECK_LAUNCH("inf_embed_kernel");
  return ROVIT_OK;
}

extern "C" size_t rovit_influence_workspace_bytes(int batch, int n, int dim, int k) {
  return search_limits_ok(batch, n, dim, k) ? keys_bytes(batch, plan_of(batch, n, k, 0)) : 0;
}

extern "C" int rovit_influence_search(const rovit_influence_query* p, rovit_stream_t stream) {
  const char* who = "influence_search";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->batch >= 1, ROVIT_ERR_SHAPE, "%s: batch %d (>= 1)", who, p->batch);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_KAN_STATS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_KAN_STATS_MAX_ROWS);
  ROVIT_CHECK_ARG(p->dim >= 32 && p->dim <= ROVIT_INFLUENCE_MAX_DIM && p->dim % 32 == 0, ROVIT_ERR_SHAPE, "%s: dim %d (a multiple of 32 in 32..%d)",
                  who, p->dim, ROVIT_INFLUENCE_MAX_DIM);
  ROVIT_CHECK_ARG(p->k >= 1 && p->k <= MAXK, ROVIT_ERR_SHAPE, "%s: k %d (1..%d)", who, p->k, MAXK);
  ROVIT_CHECK_ARG(p->relative == 0 || p->relative == 1, ROVIT_ERR_SHAPE, "%s: relative %d (0 or 1)", who, p->relative);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0 && p->max_splits >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d, max_splits %d (>= 0)", who,
                  p->max_workgroups, p->max_splits);
  ROVIT_CHECK_ARG(p->queries && p->rows && p->norm2 && p->valid && p->workspace, ROVIT_ERR_NULL, "%s: a null pointer among the inputs", who);
  ROVIT_CHECK_ARG(p->pro_scores && p->pro_indices && p->opp_scores && p->opp_indices, ROVIT_ERR_NULL, "%s: an output is missing (null pointer)", who);
  ROVIT_CHECK_ARG((p->pro_labels != nullptr) == (p->ref_labels != nullptr) && (p->opp_labels != nullptr) == (p->ref_labels != nullptr), ROVIT_ERR_NULL,
                  "%s: pro_labels and opp_labels go with ref_labels", who);
  ROVIT_CHECK_ARG((p->pro_severities != nullptr) == (p->ref_severity != nullptr) && (p->opp_severities != nullptr) == (p->ref_severity != nullptr),
                  ROVIT_ERR_NULL, "%s: pro_severities and opp_severities go with ref_severity", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->queries) && rovit_aligned16(p->rows) && rovit_aligned16(p->workspace), ROVIT_ERR_ALIGN,
                  "%s: the queries, the rows or the workspace are not 16-byte aligned", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->query_valid, 4) && rovit_aligned(p->norm2, 4) && rovit_aligned(p->valid, 4) && rovit_aligned(p->exclude, 4) &&
                      rovit_aligned(p->ref_labels, 4) && rovit_aligned(p->ref_severity, 4) && rovit_aligned(p->pro_scores, 4) &&
                      rovit_aligned(p->pro_indices, 4) && rovit_aligned(p->opp_scores, 4) && rovit_aligned(p->opp_indices, 4) &&
                      rovit_aligned(p->pro_labels, 4) && rovit_aligned(p->opp_labels, 4) && rovit_aligned(p->pro_severities, 4) &&
                      rovit_aligned(p->opp_severities, 4),
                  ROVIT_ERR_ALIGN, "%s: an array is not aligned to its element size", who);
  const int B = p->batch, n = p->n;
  const Plan pl = plan_of(B, n, p->k, p->max_splits);
  const size_t need = keys_bytes(B, pl);
  ROVIT_CHECK_ARG(p->workspace_bytes >= need, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  auto grid = [&](long long items) { return rovit_grid(items, p->max_workgroups); };
  SearchArgs a;
  a.B = B; a.n = n; a.dim = p->dim; a.relative = p->relative;
  a.qtiles = pl.qtiles; a.rtiles = pl.rtiles; a.splits = pl.splits; a.tps = pl.tps;
  a.q = p->queries; a.qok = p->query_valid; a.r = p->rows; a.rnorm = p->norm2; a.rok = p->valid; a.exclude = p->exclude;
  a.keys = (u64*)p->workspace;
  const size_t lds = search_lds_bytes(pl.kb);
  const dim3 sgrid = grid((long long)pl.qtiles * pl.splits);
  const bool ok = pl.kb == 8 ? launch_search<8>(sgrid, lds, s, a) : (pl.kb == 16 ? launch_search<16>(sgrid, lds, s, a) : launch_search<32>(sgrid, lds, s, a));
  ROVIT_CHECK_ARG(ok, ROVIT_ERR_LAUNCH, "%s: cannot raise the LDS limit", who);
  ROVIT_CHECK_LAUNCH("inf_search_kernel");
  hipLaunchKernelGGL(inf_merge_kernel, grid(2ll * B), dim3(64), merge_lds_bytes(pl.splits, pl.kb), s, *p, (const u64*)a.keys, pl.splits, pl.kb);
  ROVIT_CHECK_LAUNCH("inf_merge_kernel");
  return ROVIT_OK;
}
