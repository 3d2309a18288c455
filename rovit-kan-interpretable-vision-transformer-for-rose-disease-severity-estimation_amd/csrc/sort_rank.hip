// Device radix sort of fp32 columns and the ranks read off the sorted keys (rovit_sort_f32, rovit_rank_f32, and the internal entry
// points of sort_device.h that rovit_eval_finalize_ex, rovit_eval_selective_ex and rovit_ood_metrics_ex launch).
//
// The sorted element is the pair (key, row); (key << 32) | row has no duplicates, so the ascending order is unique and any correct
// algorithm, grid and run writes the same bytes.  LSD radix sort, four passes of 8 bits; a pass is three launches on the caller's stream:
//   sort_hist_kernel     per tile of TILE rows: the 256 digit counts in LDS (integer atomics: only the sum matters), written to the
//                        column's (digit, tile) table; the column's digit totals by integer atomics, for the same reason.
//   sort_scan_kernel     per (column, digit): the digits below it summed from the totals (a fixed tree), then the exclusive prefix sums
//                        of the digit's row of the table over the tiles (two tiles per thread, Kogge-Stone in LDS), in place.
//   sort_scatter_kernel  per tile: wave w owns rows [512 w, 512 w + 512) of the tile and walks them in 8 rounds of 64; a row's place among
//                        the rows of its digit inside its (wave, round) group is the number of lower lanes of the group with the same
//                        digit (eight ballots); the lowest such lane writes the group's count of the digit; thread d then turns the 32
//                        group counts of digit d into exclusive prefix sums in tile order.  destination = scanned table entry + group
//                        prefix + place in the group.  No atomic claims a slot: the pass is stable by construction.
// Pass 0 reads the floats and makes the keys; the passes alternate between the workspace and the caller's outputs and the fourth lands
// in the outputs.  No kernel waits for another workgroup.  Every loop is bounded by n or a constant, every destination is checked
// against n before the store, and only integers are compared.  Work items (tiles, (column, digit) pairs, 256-row chunks) are walked with
// a stride of the grid and no item's result depends on the workgroup that computes it: the grid cap changes nothing.
#include "common.h"
#include "rank_count.h"
#include "sort_device.h"

namespace {

constexpr int NT = 256;                          // threads per workgroup
constexpr int MC = ROVIT_SORT_MAX_COLUMNS;
constexpr int TILE = ROVIT_SORT_TILE;            // rows per tile
constexpr int ROUNDS = TILE / NT;                // rows per thread
constexpr int GROUPS = TILE / 64;                // (wave, round) groups of a tile, in tile order
constexpr int MAX_TILES = ROVIT_EVAL_MAX_ROWS / TILE;
static_assert(NT == RANK_NT, "rank_stage_tile strides by RANK_NT");
static_assert(MAX_TILES <= 2 * NT, "sort_scan_kernel scans two tiles per thread");
static_assert(ROUNDS * 64 * (NT / 64) == TILE && GROUPS == ROUNDS * (NT / 64), "a wave owns ROUNDS runs of 64 rows");

struct SortArgs {
  int cols, total_tiles;
  int n[MC];
  int tile0[MC + 1];                             // first tile of every column; tile0[cols] = total_tiles
  const float* x[MC];
  unsigned* out_keys[MC];
  unsigned* out_rows[MC];
  size_t off[MC];                                // the column's first element inside tmp_keys / tmp_rows
  unsigned* tmp_keys;
  unsigned* tmp_rows;
  unsigned* table;                               // column c: 256 * tile0[c] + digit * tiles_c + tile
  unsigned* totals;                              // (4 passes, cols, 256), zeroed by the caller
};

struct Layout { size_t keys, rows, table, totals, total; };
inline bool sort_limits_ok(const int* n, int cols) {
  if (!n || cols < 1 || cols > MC) return false;
  for (int c = 0; c < cols; ++c)
    if (n[c] < 1 || n[c] > ROVIT_EVAL_MAX_ROWS) return false;
  return true;
}
inline Layout sort_layout(const int* n, int cols) {
  size_t rows = 0, tiles = 0;
  for (int c = 0; c < cols; ++c) {
    rows += (size_t)n[c];
    tiles += ((size_t)n[c] + TILE - 1) / TILE;
  }
  Layout l;
  l.keys = 0;
  l.rows = l.keys + rovit_up16(rows * 4);
  l.table = l.rows + rovit_up16(rows * 4);
  l.totals = l.table + rovit_up16(tiles * 256 * 4);
  l.total = l.totals + rovit_up16((size_t)4 * cols * 256 * 4);
  return l;
}

__device__ __forceinline__ int tile_column(const SortArgs& a, int w) {
  int c = 0;
#pragma unroll
  for (int k = 1; k < MC; ++k) c += k < a.cols && w >= a.tile0[k];
  return c;
}
// where pass p reads: the floats (pass 0), the workspace (1, 3) or the outputs (2)
__device__ __forceinline__ void pass_source(const SortArgs& a, int c, int pass, const unsigned*& keys, const unsigned*& rows) {
  keys = (pass & 1) ? a.tmp_keys + a.off[c] : a.out_keys[c];
  rows = (pass & 1) ? a.tmp_rows + a.off[c] : a.out_rows[c];
}

__global__ __launch_bounds__(NT) void sort_hist_kernel(const SortArgs a, int pass) {
  __shared__ unsigned s_hist[256];
  const int tid = threadIdx.x, shift = 8 * pass;
  for (int w = blockIdx.x; w < a.total_tiles; w += gridDim.x) {
    const int c = tile_column(a, w), t = w - a.tile0[c], n = a.n[c], tiles = a.tile0[c + 1] - a.tile0[c];
    const unsigned *keys, *rows;
    pass_source(a, c, pass, keys, rows);
    __syncthreads();
    s_hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const int i = t * TILE + r * NT + tid;
      if (i < n) {
        const unsigned k = pass == 0 ? sort_key(a.x[c][i]) : keys[i];
        atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    const unsigned cnt = s_hist[tid];
    a.table[(size_t)256 * a.tile0[c] + (size_t)tid * tiles + t] = cnt;
    if (cnt) atomicAdd(&a.totals[((size_t)pass * a.cols + c) * 256 + tid], cnt);
  }
}

__global__ __launch_bounds__(NT) void sort_scan_kernel(const SortArgs a, int pass) {
  __shared__ unsigned s_u[4];
  __shared__ unsigned s_scan[NT];
  const int tid = threadIdx.x, items = a.cols * 256;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int c = w >> 8, d = w & 255, tiles = a.tile0[c + 1] - a.tile0[c];
    const unsigned base = block_sum_t(tid < d ? a.totals[((size_t)pass * a.cols + c) * 256 + tid] : 0u, s_u);
    unsigned* row = a.table + (size_t)256 * a.tile0[c] + (size_t)d * tiles;
    const int e0 = 2 * tid, e1 = 2 * tid + 1;
    const unsigned v0 = e0 < tiles ? row[e0] : 0u, v1 = e1 < tiles ? row[e1] : 0u;
    __syncthreads();
    s_scan[tid] = v0 + v1;
    __syncthreads();
    for (int s = 1; s < NT; s <<= 1) {
      const unsigned u = tid >= s ? s_scan[tid - s] : 0u;
      __syncthreads();
      s_scan[tid] += u;
      __syncthreads();
    }
    const unsigned excl = base + s_scan[tid] - (v0 + v1);
    if (e0 < tiles) row[e0] = excl;
    if (e1 < tiles) row[e1] = excl + v0;
  }
}

__global__ __launch_bounds__(NT) void sort_scatter_kernel(const SortArgs a, int pass) {
  __shared__ unsigned s_grp[GROUPS * 256];       // [group][digit]: the group's count of the digit, then its prefix inside the tile
  __shared__ unsigned s_base[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, shift = 8 * pass;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int w = blockIdx.x; w < a.total_tiles; w += gridDim.x) {
    const int c = tile_column(a, w), t = w - a.tile0[c], n = a.n[c], tiles = a.tile0[c + 1] - a.tile0[c];
    const unsigned *keys, *rows;
    pass_source(a, c, pass, keys, rows);
    unsigned* dst_keys = (pass & 1) ? a.out_keys[c] : a.tmp_keys + a.off[c];
    unsigned* dst_rows = (pass & 1) ? a.out_rows[c] : a.tmp_rows + a.off[c];
    __syncthreads();                              // the previous tile's readers of s_grp and s_base
    for (int k = tid; k < GROUPS * 256; k += NT) s_grp[k] = 0;
    s_base[tid] = a.table[(size_t)256 * a.tile0[c] + (size_t)tid * tiles + t];
    __syncthreads();
    unsigned key[ROUNDS], row[ROUNDS], place[ROUNDS];
    bool valid[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const int i = t * TILE + (wave * ROUNDS + r) * 64 + lane;
      valid[r] = i < n;
      key[r] = 0;
      row[r] = (unsigned)i;
      if (valid[r]) {
        key[r] = pass == 0 ? sort_key(a.x[c][i]) : keys[i];
        if (pass != 0) row[r] = rows[i];
      }
      const unsigned d = (key[r] >> shift) & 255u;
      unsigned long long same = __ballot(valid[r]);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const unsigned long long m = __ballot((d >> b) & 1u);
        same &= ((d >> b) & 1u) ? m : ~m;
      }
      place[r] = (unsigned)__popcll(same & below);
      if (valid[r] && place[r] == 0) s_grp[(wave * ROUNDS + r) * 256 + d] = (unsigned)__popcll(same);
    }
    __syncthreads();
    unsigned run = 0;
#pragma unroll 8
    for (int g = 0; g < GROUPS; ++g) {            // thread tid owns digit tid: groups in tile order
      const unsigned cnt = s_grp[g * 256 + tid];
      s_grp[g * 256 + tid] = run;
      run += cnt;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const unsigned d = (key[r] >> shift) & 255u;
      const unsigned dst = s_base[d] + s_grp[(wave * ROUNDS + r) * 256 + d] + place[r];
      if (valid[r] && dst < (unsigned)n) {        // always, when the table holds this pass's counts
        dst_keys[dst] = key[r];
        dst_rows[dst] = row[r];
      }
    }
  }
}

// ---- ranks ---------------------------------------------------------------------------------------------------------------------------

struct SearchArgs {
  int queries, total_chunks;
  int chunk0[MC + 1];
  RovitRankQuery q[MC];
};
struct SlotArgs {
  int cols, total_chunks;
  int chunk0[MC + 1];
  RovitRankSlots c[MC];
};
struct CountArgs {
  int cols, total_chunks;
  int chunk0[MC + 1];
  int n[MC];
  const float* x[MC];
  unsigned* less[MC];
  unsigned* eq[MC];
  unsigned* before[MC];
  unsigned* perm[MC];
};

__device__ __forceinline__ int chunk_owner(const int* chunk0, int count, int w) {
  int c = 0;
#pragma unroll
  for (int k = 1; k < MC; ++k) c += k < count && w >= chunk0[k];
  return c;
}

__global__ __launch_bounds__(NT) void rank_search_kernel(const SearchArgs a) {
  for (int w = blockIdx.x; w < a.total_chunks; w += gridDim.x) {
    const int qi = chunk_owner(a.chunk0, a.queries, w);
    const RovitRankQuery& q = a.q[qi];
    const int i = (w - a.chunk0[qi]) * NT + threadIdx.x;
    if (i < q.n) {
      const unsigned k = sort_key(q.x[i]);
      unsigned less = 0, eq = 0;
      if (k != ROVIT_SORT_NAN_KEY) {
        less = lower_bound(q.sorted, (unsigned)q.m, k);
        eq = upper_bound(q.sorted, (unsigned)q.m, k) - less;
      }
      q.less[i] = less;
      q.eq[i] = eq;
    }
  }
}

__global__ __launch_bounds__(NT) void rank_slots_kernel(const SlotArgs a) {
  for (int w = blockIdx.x; w < a.total_chunks; w += gridDim.x) {
    const int ci = chunk_owner(a.chunk0, a.cols, w);
    const RovitRankSlots& c = a.c[ci];
    const int j = (w - a.chunk0[ci]) * NT + threadIdx.x;
    if (j < c.n) {
      const unsigned k = c.keys[j], row = c.perm[j];
      if (row < (unsigned)c.n) {                  // always, behind the sort
        unsigned less = 0, eq = 0, before = 0;
        if (k != ROVIT_SORT_NAN_KEY) {
          less = lower_bound(c.keys, (unsigned)c.n, k);
          eq = upper_bound(c.keys, (unsigned)c.n, k) - less;
          before = (unsigned)j - less;
        }
        c.less[row] = less;
        c.eq[row] = eq;
        c.before[row] = before;
      }
    }
  }
}

// ROVIT_RANK_COUNT of rovit_rank_f32: sel_rank_kernel's loop over the whole j range (no split, so plain stores and no memset), and
// perm[less + before] = row in the same thread.  A NaN row counts nothing; its slot behind the numbers, #{numbers} + #{earlier NaN rows},
// is counted on the keys in a loop of its own.
__global__ __launch_bounds__(NT) void rank_count_kernel(const CountArgs a) {
  __shared__ __attribute__((aligned(16))) float sX[RANK_RT];
  const int tid = threadIdx.x;
  for (int w = blockIdx.x; w < a.total_chunks; w += gridDim.x) {
    const int c = chunk_owner(a.chunk0, a.cols, w), n = a.n[c];
    const float* X = a.x[c];
    const int i0 = (w - a.chunk0[c]) * NT, i = i0 + tid;
    const float xi = i < n ? X[i] : 0.f;
    unsigned less = 0, eq = 0, before = 0;
    const int ntiles = (n + RANK_RT - 1) / RANK_RT;
    for (int t = 0; t < ntiles; ++t) {
      __syncthreads();
      const int j0 = t * RANK_RT;
      rank_stage_tile(sX, X, j0, n);
      __syncthreads();
      unsigned e = 0;
      if (j0 + RANK_RT <= i0 || j0 >= i0 + NT) {
        rank_count_tile(sX, xi, less, e);
        if (j0 + RANK_RT <= i0) before += e;
      } else {
        rank_count_tile<true>(sX, xi, less, e, &before, i - j0);
      }
      eq += e;
    }
    if (i < n) {
      unsigned slot = less + before;
      if (sort_key(xi) == ROVIT_SORT_NAN_KEY) {
        slot = 0;
        for (int j = 0; j < n; ++j) slot += (sort_key(X[j]) != ROVIT_SORT_NAN_KEY) | (j < i);
      }
      a.less[c][i] = less;
      a.eq[c][i] = eq;
      a.before[c][i] = before;
      if (slot < (unsigned)n) a.perm[c][slot] = (unsigned)i;
    }
  }
}

inline dim3 capped(long long items, int max_workgroups) {
  const long long cap = max_workgroups > 0 ? max_workgroups : (1ll << 30);
  return dim3((unsigned)(items < cap ? items : cap));
}

}  // namespace

size_t rovit_sort_batch_workspace_bytes(const int* n, int cols) { return sort_limits_ok(n, cols) ? sort_layout(n, cols).total : 0; }

int rovit_sort_batch(const RovitSortCol* c, int cols, void* workspace, size_t workspace_bytes, int max_workgroups, hipStream_t stream,
                     const char* who) {
  int n[MC];
  ROVIT_CHECK_ARG(c && cols >= 1 && cols <= MC, ROVIT_ERR_SHAPE, "%s: %d columns to sort (1..%d)", who, cols, MC);
  for (int k = 0; k < cols; ++k) {
    ROVIT_CHECK_ARG(c[k].n >= 1 && c[k].n <= ROVIT_EVAL_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: column %d has %d rows (1..%d)", who, k, c[k].n,
                    ROVIT_EVAL_MAX_ROWS);
    ROVIT_CHECK_ARG(c[k].x && c[k].keys && c[k].perm, ROVIT_ERR_NULL, "%s: column %d has a null pointer", who, k);
    ROVIT_CHECK_ARG(rovit_aligned(c[k].x, 4) && rovit_aligned(c[k].keys, 4) && rovit_aligned(c[k].perm, 4), ROVIT_ERR_ALIGN,
                    "%s: an array of column %d is not aligned to its element size", who, k);
    n[k] = c[k].n;
  }
  ROVIT_CHECK_ARG(max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, max_workgroups);
  const Layout l = sort_layout(n, cols);
  ROVIT_CHECK_ARG(workspace, ROVIT_ERR_NULL, "%s: the sort's workspace is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned16(workspace), ROVIT_ERR_ALIGN, "%s: the sort's workspace is not 16-byte aligned", who);
  ROVIT_CHECK_ARG(workspace_bytes >= l.total, ROVIT_ERR_SHAPE, "%s: the sort's workspace holds %zu bytes, %zu are needed", who, workspace_bytes,
                  l.total);
  char* ws = (char*)workspace;
  SortArgs a;
  a.cols = cols;
  size_t off = 0;
  int tile = 0;
  for (int k = 0; k < MC; ++k) {
    const bool on = k < cols;
    a.n[k] = on ? c[k].n : 0;
    a.x[k] = on ? c[k].x : nullptr;
    a.out_keys[k] = on ? c[k].keys : nullptr;
    a.out_rows[k] = on ? c[k].perm : nullptr;
    a.tile0[k] = tile;
    a.off[k] = off;
    if (on) {
      tile += (c[k].n + TILE - 1) / TILE;
      off += (size_t)c[k].n;
    }
  }
  a.tile0[MC] = tile;
  for (int k = cols; k < MC; ++k) a.tile0[k] = tile;
  a.total_tiles = tile;
  a.tmp_keys = (unsigned*)(ws + l.keys);
  a.tmp_rows = (unsigned*)(ws + l.rows);
  a.table = (unsigned*)(ws + l.table);
  a.totals = (unsigned*)(ws + l.totals);
  if (hipMemsetAsync(a.totals, 0, l.total - l.totals, stream) != hipSuccess) {
    rovit_set_error("%s: hipMemsetAsync failed", who);
    return ROVIT_ERR_LAUNCH;
  }
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(sort_hist_kernel, capped(a.total_tiles, max_workgroups), dim3(NT), 0, stream, a, pass);
    ROVIT_CHECK_LAUNCH("sort_hist_kernel");
    hipLaunchKernelGGL(sort_scan_kernel, capped((long long)cols * 256, max_workgroups), dim3(NT), 0, stream, a, pass);
    ROVIT_CHECK_LAUNCH("sort_scan_kernel");
    hipLaunchKernelGGL(sort_scatter_kernel, capped(a.total_tiles, max_workgroups), dim3(NT), 0, stream, a, pass);
    ROVIT_CHECK_LAUNCH("sort_scatter_kernel");
  }
  return ROVIT_OK;
}

int rovit_rank_search(const RovitRankQuery* q, int queries, int max_workgroups, hipStream_t stream, const char* who) {
  ROVIT_CHECK_ARG(q && queries >= 1 && queries <= MC, ROVIT_ERR_SHAPE, "%s: %d rank queries (1..%d)", who, queries, MC);
  SearchArgs a;
  a.queries = queries;
  int chunk = 0;
  for (int k = 0; k < MC; ++k) {
    a.chunk0[k] = chunk;
    if (k < queries) {
      ROVIT_CHECK_ARG(q[k].x && q[k].sorted && q[k].less && q[k].eq && q[k].n >= 1 && q[k].m >= 1 && q[k].n <= ROVIT_EVAL_MAX_ROWS &&
                          q[k].m <= ROVIT_EVAL_MAX_ROWS,
                      ROVIT_ERR_SHAPE, "%s: rank query %d is malformed", who, k);
      a.q[k] = q[k];
      chunk += (q[k].n + NT - 1) / NT;
    } else {
      a.q[k] = RovitRankQuery{nullptr, 0, nullptr, 0, nullptr, nullptr};
    }
  }
  a.chunk0[MC] = chunk;
  a.total_chunks = chunk;
  hipLaunchKernelGGL(rank_search_kernel, capped(chunk, max_workgroups), dim3(NT), 0, stream, a);
  ROVIT_CHECK_LAUNCH("rank_search_kernel");
  return ROVIT_OK;
}

int rovit_rank_slots(const RovitRankSlots* c, int cols, int max_workgroups, hipStream_t stream, const char* who) {
  ROVIT_CHECK_ARG(c && cols >= 1 && cols <= MC, ROVIT_ERR_SHAPE, "%s: %d sorted columns (1..%d)", who, cols, MC);
  SlotArgs a;
  a.cols = cols;
  int chunk = 0;
  for (int k = 0; k < MC; ++k) {
    a.chunk0[k] = chunk;
    if (k < cols) {
      ROVIT_CHECK_ARG(c[k].keys && c[k].perm && c[k].less && c[k].eq && c[k].before && c[k].n >= 1 && c[k].n <= ROVIT_EVAL_MAX_ROWS,
                      ROVIT_ERR_SHAPE, "%s: sorted column %d is malformed", who, k);
      a.c[k] = c[k];
      chunk += (c[k].n + NT - 1) / NT;
    } else {
      a.c[k] = RovitRankSlots{nullptr, nullptr, 0, nullptr, nullptr, nullptr};
    }
  }
  a.chunk0[MC] = chunk;
  a.total_chunks = chunk;
  hipLaunchKernelGGL(rank_slots_kernel, capped(chunk, max_workgroups), dim3(NT), 0, stream, a);
  ROVIT_CHECK_LAUNCH("rank_slots_kernel");
  return ROVIT_OK;
}

extern "C" size_t rovit_sort_workspace_bytes(const int* n, int num_columns) { return rovit_sort_batch_workspace_bytes(n, num_columns); }

extern "C" int rovit_sort_f32(const rovit_sort* p, rovit_stream_t stream) {
  const char* who = "sort_f32";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->num_columns >= 1 && p->num_columns <= MC, ROVIT_ERR_SHAPE, "%s: %d columns (1..%d)", who, p->num_columns, MC);
  RovitSortCol c[MC];
  for (int k = 0; k < p->num_columns; ++k) c[k] = RovitSortCol{p->x[k], p->keys_sorted[k], p->perm[k], p->n[k]};
  return rovit_sort_batch(c, p->num_columns, p->workspace, p->workspace_bytes, p->max_workgroups, (hipStream_t)stream, who);
}

namespace {
struct RankLayout { size_t keys, sort, total; };
inline RankLayout rank_layout(const int* n, int cols) {
  size_t rows = 0;
  for (int c = 0; c < cols; ++c) rows += rovit_up16((size_t)n[c] * 4);
  RankLayout l;
  l.keys = 0;
  l.sort = rows;
  l.total = l.sort + sort_layout(n, cols).total;
  return l;
}
}  // namespace

extern "C" size_t rovit_rank_workspace_bytes(const int* n, int num_columns, int method) {
  if (!sort_limits_ok(n, num_columns) || method < ROVIT_RANK_AUTO || method > ROVIT_RANK_SORT) return 0;
  int longest = 0;
  for (int c = 0; c < num_columns; ++c) longest = n[c] > longest ? n[c] : longest;
  return rovit_rank_method(method, longest) == ROVIT_RANK_SORT ? rank_layout(n, num_columns).total : 0;
}

extern "C" int rovit_rank_f32(const rovit_rank* p, rovit_stream_t stream) {
  const char* who = "rank_f32";
  ROVIT_CHECK_ARG(p, ROVIT_ERR_NULL, "%s: null descriptor", who);
  ROVIT_CHECK_ARG(p->num_columns >= 1 && p->num_columns <= MC, ROVIT_ERR_SHAPE, "%s: %d columns (1..%d)", who, p->num_columns, MC);
  ROVIT_CHECK_ARG(p->method >= ROVIT_RANK_AUTO && p->method <= ROVIT_RANK_SORT, ROVIT_ERR_SHAPE, "%s: unknown method %d", who, p->method);
  ROVIT_CHECK_ARG(p->max_workgroups >= 0, ROVIT_ERR_SHAPE, "%s: max_workgroups %d (>= 0)", who, p->max_workgroups);
  const int cols = p->num_columns;
  int longest = 0;
  for (int k = 0; k < cols; ++k) {
    ROVIT_CHECK_ARG(p->n[k] >= 1 && p->n[k] <= ROVIT_EVAL_MAX_ROWS, ROVIT_ERR_SHAPE, "%s: column %d has %d rows (1..%d)", who, k, p->n[k],
                    ROVIT_EVAL_MAX_ROWS);
    ROVIT_CHECK_ARG(p->x[k] && p->less[k] && p->eq[k] && p->before[k] && p->perm[k], ROVIT_ERR_NULL, "%s: column %d has a null pointer", who, k);
    ROVIT_CHECK_ARG(rovit_aligned(p->x[k], 4) && rovit_aligned(p->less[k], 4) && rovit_aligned(p->eq[k], 4) && rovit_aligned(p->before[k], 4) &&
                        rovit_aligned(p->perm[k], 4),
                    ROVIT_ERR_ALIGN, "%s: an array of column %d is not aligned to its element size", who, k);
    longest = p->n[k] > longest ? p->n[k] : longest;
  }
  hipStream_t s = (hipStream_t)stream;
  if (rovit_rank_method(p->method, longest) == ROVIT_RANK_COUNT) {
    CountArgs a;
    a.cols = cols;
    int chunk = 0;
    for (int k = 0; k < MC; ++k) {
      const bool on = k < cols;
      a.chunk0[k] = chunk;
      a.n[k] = on ? p->n[k] : 0;
      a.x[k] = on ? p->x[k] : nullptr;
      a.less[k] = on ? p->less[k] : nullptr;
      a.eq[k] = on ? p->eq[k] : nullptr;
      a.before[k] = on ? p->before[k] : nullptr;
      a.perm[k] = on ? p->perm[k] : nullptr;
      if (on) chunk += (p->n[k] + NT - 1) / NT;
    }
    a.chunk0[MC] = chunk;
    a.total_chunks = chunk;
    hipLaunchKernelGGL(rank_count_kernel, capped(chunk, p->max_workgroups), dim3(NT), 0, s, a);
    ROVIT_CHECK_LAUNCH("rank_count_kernel");
    return ROVIT_OK;
  }
  const RankLayout l = rank_layout(p->n, cols);
  ROVIT_CHECK_ARG(p->workspace, ROVIT_ERR_NULL, "%s: the workspace is missing (null pointer)", who);
  ROVIT_CHECK_ARG(rovit_aligned16(p->workspace), ROVIT_ERR_ALIGN, "%s: the workspace is not 16-byte aligned", who);
  ROVIT_CHECK_ARG(p->workspace_bytes >= l.total, ROVIT_ERR_SHAPE, "%s: the workspace holds %zu bytes, %zu are needed", who, p->workspace_bytes,
                  l.total);
  char* ws = (char*)p->workspace;
  RovitSortCol c[MC];
  RovitRankSlots r[MC];
  size_t off = 0;
  for (int k = 0; k < cols; ++k) {
    unsigned* keys = (unsigned*)(ws + l.keys + off);
    off += rovit_up16((size_t)p->n[k] * 4);
    c[k] = RovitSortCol{p->x[k], keys, p->perm[k], p->n[k]};
    r[k] = RovitRankSlots{keys, p->perm[k], p->n[k], p->less[k], p->eq[k], p->before[k]};
  }
  const int rc = rovit_sort_batch(c, cols, ws + l.sort, p->workspace_bytes - l.sort, p->max_workgroups, s, who);
  if (rc != ROVIT_OK) return rc;
  return rovit_rank_slots(r, cols, p->max_workgroups, s, who);
}
