// Nearest neighbours in feature space on the device: the k nearest recorded feature rows of every query row (rovit_knn_build,
// rovit_knn_search) and the neighbour-weighted vote on top.  The recipe `q @ r.T` + `torch.topk` materialises a (batch, n) matrix and has
// no tie rule; here no such matrix exists, the order is total, and the answer is the same bits for every grid and split.
//
// Distance (include/rovit_hip.h): l2 = max(0, (|q|^2 + |r|^2) - 2 q.r), cosine = max(0, 1 - q^.r^); every term fp32, q.r and the norms
// fma chains in ascending feature index.  q.r runs on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32: a k-ordered fp32 fma
// chain; feature_tiles.h), so a distance is a function of its two rows alone.  Order: the key (bits(d) << 32) | j as an unsigned
// 64-bit integer; the k smallest keys, ascending.  Only integer compares decide membership.
//
//   knn_rows_kernel    a thread per row: the row scan of feature_tiles.h (squared norm, validity flag; for the recorded rows with cosine
//                      also the normalised copy) and the integer counts (integer atomics).
//   knn_search_kernel  a work item = (query tile of 64 rows, reference split).  The 64 query rows sit in LDS (normalised on the way in with
//                      cosine); 64-row reference tiles stream through a second LDS buffer, the next tile's loads in flight in registers while
//                      this tile's products run.  Both buffers hold each group of 8 features as (f0 f2 f4 f6 | f1 f3 f5 f7): a lane half
//                      reads one float4 and the four matrix instructions of a group then see k = (f0, f1), (f2, f3), ...: ascending.
//                      Wave (qt, rt) forms the 32 x 32 block of query tile qt against reference sub-tile rt with the queries on the lane
//                      index: a lane holds 16 reference distances of ONE query, and keeps its own ascending list of KB keys in registers
//                      (fully unrolled).  A candidate enters the compare-exchange chain only when its key is below the list's last, and
//                      the wave skips the chain when no lane has such a candidate.  The four lists of a query (two lane halves, two waves)
//                      meet in LDS; every key's rank among them is its index in its own list plus a binary search in the three others,
//                      and the KB smallest go to the workspace.
//   knn_merge_kernel   a wave per query: the splits' lists to LDS; only the keys up to a threshold (the smaller of the smallest k-th key of any
//                      one split and the k-th smallest first key) are ranked, a lane per split and an integer sum over the wave; the k
//                      smallest unpacked; then the vote in fp64 in slot order by one lane.
// Work items are walked with a stride of the grid; no floating-point atomic; no result depends on which workgroup computes it.
#include "common.h"
#include "feature_tiles.h"
#include "topk_device.h"

namespace {

using namespace ftile;                           // row_scan, count_rows, store_unit, tile_dot, acc_row, dist_of
using namespace topk;                            // u64, EMPTY, key_of, keys_below, list_insert, merge_four, Plan, plan_of

constexpr int NT = 256;                        // threads per workgroup
constexpr int QT = ROVIT_KNN_QUERY_TILE;         // query rows of a work item
constexpr int RT = 64;                           // reference rows of an LDS tile
constexpr int MAXK = ROVIT_KNN_MAX_K;
constexpr int MAX_T = 8;                         // embed / 32
static_assert(QT == 64 && RT == 64, "2 x 2 sub-tiles of 32 per workgroup, one per wave; plan_of's tiles");

struct Layout { size_t qnorm, qok, keys, total; };
inline Layout layout_of(int B, const Plan& p) {
  Layout l;
  l.qnorm = 0;
  l.qok = l.qnorm + rovit_up16((size_t)B * 4);
  l.keys = l.qok + rovit_up16((size_t)B * 4);
  l.total = l.keys + rovit_up16((size_t)B * p.splits * p.kb * 8);
  return l;
}

inline bool limits_ok(int B, int N, int E, int k) {
  return B >= 1 && N >= 1 && N <= ROVIT_KAN_STATS_MAX_ROWS && E >= 32 && E <= 256 && E % 32 == 0 && k >= 1 && k <= MAXK;
}

// ---- rows: norms, flags, the normalised copy -------------------------------------------------------------------------------------------

struct RowArgs {
  int n, E, cosine;
  const float* x;
  float* norm;
  int* ok;
  float* xhat;              // or nullptr
  u64* counts;              // or nullptr: [ROVIT_KNN_N], [_N_VALID], [_BAD_ROWS], zeroed before the launch
};

__global__ __launch_bounds__(NT) void knn_rows_kernel(const RowArgs a) {
  const int chunks = (a.n + NT - 1) / NT;
  for (int w = blockIdx.x; w < chunks; w += gridDim.x) {
    const int row = w * NT + threadIdx.x;
    bool good = false;
    if (row < a.n) good = row_scan(a.x, a.norm, a.ok, a.xhat, row, a.E, a.cosine);
    if (a.counts) count_rows(a.counts, good, row, a.n, ROVIT_KNN_N, ROVIT_KNN_N_VALID, ROVIT_KNN_BAD_ROWS);
  }
}

// ---- search ----------------------------------------------------------------------------------------------------------------------------

struct SearchArgs {
  int B, N, E, cosine, qtiles, rtiles, splits, tps;
  const float* q;
  const float* r;
  const float* rnorm;
  const int* rok;
  const float* qnorm;
  const int* qok;
  const int* exclude;       // or nullptr
  u64* keys;                // (B, splits, KB)
};

inline size_t search_lds_bytes(int E, int kb) {
  const size_t stage = ((size_t)(QT + RT) * (E + 4) + 2 * RT) * 4, merge = (size_t)QT * 4 * kb * 8;
  return stage > merge ? stage : merge;
}

template <int KB>
__global__ __launch_bounds__(NT) void knn_search_kernel(const SearchArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int E = a.E, ST = E + 4, E8 = E / 8, T = E / 32;
  float* Qs = lds;                                               // [64][ST] query rows
  float* Rs = Qs + QT * ST;                                      // [64][ST] one reference tile
  float* s_rn = Rs + RT * ST;                                    // [64] squared norms of the tile's rows
  int* s_rj = reinterpret_cast<int*>(s_rn + RT);                 // [64] their indices, -1: not a candidate
  u64* Ms = reinterpret_cast<u64*>(lds);                         // [64][4][KB] the lists of a tile's queries, over the staging buffers
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), qtw = wv >> 1, rtw = wv & 1;
  const int items = a.qtiles * a.splits;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int qt = item % a.qtiles, sp = item / a.qtiles, q0 = qt * QT;
    __syncthreads();                                             // the previous item's lists have been read
#pragma unroll
    for (int i = 0; i < MAX_T; ++i)
      if (i < T) {
        const int idx = tid + NT * i, row = idx / E8, c8 = idx - row * E8, g = q0 + row;
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
        if (g < a.B && a.qok[g]) {
          const float4* src = reinterpret_cast<const float4*>(a.q + (size_t)g * E + 8 * c8);
          u = src[0];
          v = src[1];
          if (a.cosine) {
            const float len = sqrtf(a.qnorm[g]);
            u = make_float4(u.x / len, u.y / len, u.z / len, u.w / len);
            v = make_float4(v.x / len, v.y / len, v.z / len, v.w / len);
          }
        }
        store_unit(Qs + row * ST + 8 * c8, u, v);               // k ascending in feature index, as for the reference tiles below
      }
    const int qrow = q0 + qtw * 32 + l31;
    const bool qgood = qrow < a.B && a.qok[qrow] != 0;
    const float qn = qgood ? a.qnorm[qrow] : 0.f;
    const int excl = (qgood && a.exclude) ? a.exclude[qrow] : -1;
    u64 lst[KB];
#pragma unroll
    for (int i = 0; i < KB; ++i) lst[i] = EMPTY;
    const int t0 = sp * a.tps, t1 = min(a.rtiles, t0 + a.tps);
    float4 pu[MAX_T], pv[MAX_T];
    float p_rn = 0.f;
    int p_rj = -1;
    auto fetch = [&](int t) {                                    // tile t into registers; rows that are no candidates become zeros
      const int j0 = t * RT;
#pragma unroll
      for (int i = 0; i < MAX_T; ++i)
        if (i < T) {
          const int idx = tid + NT * i, row = idx / E8, c8 = idx - row * E8, j = j0 + row;
          pu[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          pv[i] = pu[i];
          if (j < a.N && a.rok[j]) {
            const float4* src = reinterpret_cast<const float4*>(a.r + (size_t)j * E + 8 * c8);
            pu[i] = src[0];
            pv[i] = src[1];
          }
        }
      if (tid < RT) {
        const int j = j0 + tid;
        const bool ok = j < a.N && a.rok[j] != 0;
        p_rn = ok ? a.rnorm[j] : 0.f;
        p_rj = ok ? j : -1;
      }
    };
    fetch(t0);
    for (int t = t0; t < t1; ++t) {
      __syncthreads();                                           // the previous tile's products are done (first pass: nothing to wait for)
#pragma unroll
      for (int i = 0; i < MAX_T; ++i)
        if (i < T) {
          const int idx = tid + NT * i, row = idx / E8, c8 = idx - row * E8;
          store_unit(Rs + row * ST + 8 * c8, pu[i], pv[i]);
        }
      if (tid < RT) {
        s_rn[tid] = p_rn;
        s_rj[tid] = p_rj;
      }
      __syncthreads();
      if (t + 1 < t1) fetch(t + 1);                              // in flight behind the products below
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* rrow = Rs + (rtw * 32 + l31) * ST + 4 * lh;   // A[m = reference][k]: lane half h holds feature 8 b + 2 s + h in step s
      const float* qrw = Qs + (qtw * 32 + l31) * ST + 4 * lh;    // B[k][n = query]
      acc = tile_dot(acc, rrow, qrw, E);
      // lane (l31, h) holds q.r of query l31 against the sub-tile's rows acc_row(r, h)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = rtw * 32 + acc_row(r, lh);
        const int j = s_rj[i];
        bool fin;
        const float d = dist_of(a.cosine, qn, s_rn[i], acc[r], &fin);
        const bool cand = qgood && j >= 0 && j != excl && fin;
        const u64 key = cand ? key_of(__float_as_uint(d), j) : EMPTY;
        if (__ballot(key < lst[KB - 1]) != 0ull) list_insert<KB>(lst, key);
      }
    }
    const int g = q0 + (tid >> 2);                               // the query whose four lists this thread helps to merge
    merge_four<KB>(lst, Ms, (qtw * 32 + l31) * 4 + rtw * 2 + lh, g < a.B ? a.keys + ((size_t)g * a.splits + sp) * KB : nullptr);
  }
}

// ---- merge and vote --------------------------------------------------------------------------------------------------------------------

inline size_t merge_lds_bytes(int splits, int kb, int C) { return ((size_t)splits * kb + MAXK) * 8 + (size_t)(C > 0 ? C : 1) * 8; }

__global__ __launch_bounds__(64) void knn_merge_kernel(const rovit_knn_query a, const u64* keys, int splits, int KB) {
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  u64* L = sm;                                                   // [splits][KB]
  u64* top = L + splits * KB;                                    // [MAXK]
  double* s_cls = reinterpret_cast<double*>(top + MAXK);         // [C]
  const int lane = threadIdx.x, k = a.k, total = splits * KB;
  const bool vote = a.class_probs != nullptr;
  const int C = vote ? a.num_classes : 0;
  for (int q = blockIdx.x; q < a.batch; q += gridDim.x) {
    __syncthreads();
    for (int i = lane; i < total; i += 64) L[i] = keys[(size_t)q * total + i];
    if (lane < MAXK) top[lane] = EMPTY;
    for (int c = lane; c < C; c += 64) s_cls[c] = 0.0;
    __syncthreads();
    // At least k keys lie at or below the k-th key of any one split, and at or below the k-th smallest of the splits' first keys: no key
    // above t, the smaller of the two, can be among the k smallest of all, and only the keys up to t are ranked.  A lane per split counts
    // the split's keys below the candidate (its own position for the candidate's split); the sum over the wave is the rank.
    if (splits == 1) {
      if (lane < k) top[lane] = L[lane];
    } else {
      auto wave_min = [](u64 v) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
          const u64 o = __shfl_xor(v, m);
          v = o < v ? o : v;
        }
        return v;
      };
      u64 t = EMPTY;
      for (int s = lane; s < splits; s += 64) {
        const u64 v = L[s * KB + k - 1];
        t = v < t ? v : t;
      }
      t = wave_min(t);
      if (splits >= k) {                                           // splits <= 64: a lane per first key, real first keys are distinct
        const u64 mine = lane < splits ? L[lane * KB] : EMPTY;
        int less = 0;
        for (int s = 0; s < splits; ++s) less += L[s * KB] < mine ? 1 : 0;
        const u64 t2 = wave_min(mine != EMPTY && less == k - 1 ? mine : EMPTY);
        t = t2 < t ? t2 : t;
      }
      for (int s = 0; s < splits; ++s)
        for (int p = 0; p < KB; ++p) {
          const u64 c = L[s * KB + p];                             // the same word for every lane: the loop is uniform
          if (c == EMPTY || c > t) break;
          int below = 0;
          for (int l = lane; l < splits; l += 64) below += l == s ? p : keys_below(L + l * KB, KB, c);
#pragma unroll
          for (int m = 1; m < 64; m <<= 1) below += __shfl_xor(below, m);
          if (lane == 0 && below < k) top[below] = c;
        }
    }
    __syncthreads();
    if (lane < k) {
      const u64 c = top[lane];
      const bool real = c != EMPTY;
      const int j = real ? key_index(c) : -1;
      const size_t o = (size_t)q * k + lane;
      a.distances[o] = real ? __uint_as_float(key_bits(c)) : __builtin_inff();
      a.indices[o] = j;
      if (a.labels) a.labels[o] = real ? a.ref_labels[j] : -1;
      if (a.severities) a.severities[o] = real ? a.ref_severity[j] : __builtin_nanf("");
    }
    if (lane == 0) {
      int nv = 0;
      while (nv < k && top[nv] != EMPTY) ++nv;
      double sw = 0.0, ss = 0.0, sd = 0.0, dk = 0.0;
      const double d1 = nv ? (double)__uint_as_float(key_bits(top[0])) : 0.0;
      for (int s = 0; s < nv; ++s) {
        const u64 c = top[s];
        const int j = key_index(c);
        dk = (double)__uint_as_float(key_bits(c));
        const double w = exp(-(dk - d1) / a.temperature);
        sw += w;
        sd += dk;
        if (vote) {
          const int y = a.ref_labels[j];
          if (y >= 0 && y < C) s_cls[y] += w;
        }
        if (a.severity) ss += w * (double)a.ref_severity[j];
      }
      a.kth_distance[q] = nv ? (float)dk : __builtin_inff();
      a.mean_distance[q] = nv ? (float)(sd / (double)nv) : __builtin_inff();
      if (a.severity) a.severity[q] = nv ? (float)(ss / sw) : __builtin_nanf("");
      if (vote) {
        int arg = nv ? 0 : -1;
        for (int c = 1; c < C && nv; ++c)
          if (s_cls[c] > s_cls[arg]) arg = c;
        a.cls[q] = arg;
        for (int c = 0; c < C; ++c) s_cls[c] = nv ? s_cls[c] / sw : 0.0;
      }
    }
    __syncthreads();
    for (int c = lane; c < C; c += 64) a.class_probs[(size_t)q * C + c] = (float)s_cls[c];
  }
}

template <int KB>
bool launch_search(dim3 grid, size_t lds, hipStream_t s, const SearchArgs& a) {
  if (!rovit_set_max_lds((const void*)knn_search_kernel<KB>, lds)) return false;
  hipLaunchKernelGGL(knn_search_kernel<KB>, grid, dim3(NT), lds, s, a);
  return true;
}

}  // namespace

extern "C" size_t rovit_knn_workspace_bytes(int batch, int n, int embed, int k) {
  return limits_ok(batch, n, embed, k) ? layout_of(batch, plan_of(batch, n, k, 0)).total : 0;
}

extern "C" int rovit_knn_build(const rovit_knn_index* p, rovit_stream_t stream) {
  const char* who = "knn_build";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_KAN_STATS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_KAN_STATS_MAX_ROWS);
  ROVIT_CHECK_ARG(p->embed >= 32 && p->embed <= 256 && p->embed % 32 == 0, ROVIT_ERR_SHAPE, "%s: embed %d (a multiple of 32 in 32..256)", who,
                  p->embed);
  ROVIT_CHECK_ARG(p->metric == ROVIT_KNN_L2 || p->metric == ROVIT_KNN_COSINE, ROVIT_ERR_SHAPE, "%s: metric %d", who, p->metric);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->features && p->norms && p->valid && p->result, ROVIT_ERR_NULL, "%s: a null pointer", who);
  ROVIT_CHECK_ARG((p->metric == ROVIT_KNN_COSINE) == (p->normalized != nullptr), ROVIT_ERR_NULL,
                  "%s: the normalized copy goes with the cosine metric and with no other", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->features) && rovit_aligned16(p->normalized) && rovit_aligned(p->norms, 4) && rovit_aligned(p->valid, 4) &&
                      rovit_aligned(p->result, 8),
                  ROVIT_ERR_ALIGN, "%s: the rows are not 16-byte aligned, or an array not to its words", who);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(p->result, 0, ROVIT_KNN_WORDS * 8, s) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  RowArgs a;
  a.n = p->n; a.E = p->embed; a.cosine = p->metric == ROVIT_KNN_COSINE;
  a.x = p->features; a.norm = p->norms; a.ok = p->valid; a.xhat = p->normalized; a.counts = (u64*)p->result;
  hipLaunchKernelGGL(knn_rows_kernel, rovit_grid(((long long)p->n + NT - 1) / NT, p->max_workgroups), dim3(NT), 0, s, a);
  ROVIT_CHECK_LAUNCH("knn_rows_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_knn_search(const rovit_knn_query* p, rovit_stream_t stream) {
  const char* who = "knn_search";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->batch >= 1, ROVIT_ERR_SHAPE, "%s: batch %d (>= 1)", who, p->batch);
  ROVIT_CHECK_ARG(p->n >= 1 && p->n <= ROVIT_KAN_STATS_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: %d rows (1..%d)", who, p->n, ROVIT_KAN_STATS_MAX_ROWS);
  ROVIT_CHECK_ARG(p->embed >= 32 && p->embed <= 256 && p->embed % 32 == 0, ROVIT_ERR_SHAPE, "%s: embed %d (a multiple of 32 in 32..256)", who,
                  p->embed);
  ROVIT_CHECK_ARG(p->k >= 1 && p->k <= MAXK, ROVIT_ERR_SHAPE, "%s: k %d (1..%d)", who, p->k, MAXK);
  ROVIT_CHECK_ARG(p->metric == ROVIT_KNN_L2 || p->metric == ROVIT_KNN_COSINE, ROVIT_ERR_SHAPE, "%s: metric %d", who, p->metric);
  ROVIT_CHECK_ARG(p->num_classes >= 0 && p->num_classes <= ROVIT_KNN_MAX_CLASSES, ROVIT_ERR_SHAPE, "%s: %d classes (0..%d)", who, p->num_classes,
                  ROVIT_KNN_MAX_CLASSES);
  ROVIT_CHECK_ARG(p->temperature > 0.0 && p->temperature < 1e300, ROVIT_ERR_SHAPE, "%s: temperature %g (> 0)", who, p->temperature);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  ROVIT_CHECK_ARG(p->queries && p->rows && p->norms && p->valid && p->workspace, ROVIT_ERR_NULL, "%s: a null pointer among the inputs", who);
  ROVIT_CHECK_ARG(p->distances && p->indices && p->kth_distance && p->mean_distance, ROVIT_ERR_NULL, "%s: an output is missing (null pointer)", who);
  ROVIT_CHECK_ARG((p->labels != nullptr) == (p->ref_labels != nullptr), ROVIT_ERR_NULL, "%s: labels goes with ref_labels", who);
  ROVIT_CHECK_ARG((p->severities != nullptr) == (p->ref_severity != nullptr) && (p->severity != nullptr) == (p->ref_severity != nullptr),
                  ROVIT_ERR_NULL, "%s: severities and severity go with ref_severity", who);
  ROVIT_CHECK_ARG((p->class_probs != nullptr) == (p->cls != nullptr) && (p->class_probs == nullptr || (p->ref_labels && p->num_classes >= 1)),
                  ROVIT_ERR_NULL, "%s: class_probs and cls go together, with ref_labels and num_classes >= 1", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->queries) && rovit_aligned16(p->rows) && rovit_aligned16(p->workspace), ROVIT_ERR_ALIGN,
                  "%s: the queries, the rows or the workspace are not 16-byte aligned", who);
  ROVIT_CHECK_ARG(rovit_aligned(p->norms, 4) && rovit_aligned(p->valid, 4) && rovit_aligned(p->exclude, 4) && rovit_aligned(p->ref_labels, 4) &&
                      rovit_aligned(p->ref_severity, 4) && rovit_aligned(p->distances, 4) && rovit_aligned(p->indices, 4) && rovit_aligned(p->labels, 4) &&
                      rovit_aligned(p->severities, 4) && rovit_aligned(p->class_probs, 4) && rovit_aligned(p->cls, 4) && rovit_aligned(p->severity, 4) &&
                      rovit_aligned(p->kth_distance, 4) && rovit_aligned(p->mean_distance, 4),
                  ROVIT_ERR_ALIGN, "%s: an array is not aligned to its element size", who);
  const int B = p->batch, N = p->n, E = p->embed;
  const Plan pl = plan_of(B, N, p->k, 0);
  const Layout l = layout_of(B, pl);
  ROVIT_CHECK_ARG(p->workspace_bytes >= l.total, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes,
                  l.total);
  char* ws = (char*)p->workspace;
  hipStream_t s = (hipStream_t)stream;
  auto grid = [&](long long items) { return rovit_grid(items, p->max_workgroups); };
  const bool cosine = p->metric == ROVIT_KNN_COSINE;
  RowArgs ra;
  ra.n = B; ra.E = E; ra.cosine = cosine;
  ra.x = p->queries; ra.norm = (float*)(ws + l.qnorm); ra.ok = (int*)(ws + l.qok); ra.xhat = nullptr; ra.counts = nullptr;
  hipLaunchKernelGGL(knn_rows_kernel, grid(((long long)B + NT - 1) / NT), dim3(NT), 0, s, ra);
  ROVIT_CHECK_LAUNCH("knn_rows_kernel");
  SearchArgs a;
  a.B = B; a.N = N; a.E = E; a.cosine = cosine;
  a.qtiles = pl.qtiles; a.rtiles = pl.rtiles; a.splits = pl.splits; a.tps = pl.tps;
  a.q = p->queries; a.r = p->rows; a.rnorm = p->norms; a.rok = p->valid;
  a.qnorm = ra.norm; a.qok = ra.ok; a.exclude = p->exclude;
  a.keys = (u64*)(ws + l.keys);
  const size_t lds = search_lds_bytes(E, pl.kb);
  const dim3 sgrid = grid((long long)pl.qtiles * pl.splits);
  const bool ok = pl.kb == 8 ? launch_search<8>(sgrid, lds, s, a) : (pl.kb == 16 ? launch_search<16>(sgrid, lds, s, a) : launch_search<32>(sgrid, lds, s, a));
  ROVIT_CHECK_ARG(ok, ROVIT_ERR_LAUNCH, "%s: cannot raise the LDS limit", who);
  ROVIT_CHECK_LAUNCH("knn_search_kernel");
  const size_t mlds = merge_lds_bytes(pl.splits, pl.kb, p->class_probs ? p->num_classes : 0);
  hipLaunchKernelGGL(knn_merge_kernel, grid(B), dim3(64), mlds, s, *p, (const u64*)a.keys, pl.splits, pl.kb);
  ROVIT_CHECK_LAUNCH("knn_merge_kernel");
  return ROVIT_OK;
}
