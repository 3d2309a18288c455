// Image corruptions of a device-resident uint8 image store (Hendrycks & Dietterich, ICLR 2019: fixed corruptions at five severities):
// gather by index, corrupt, clamp, normalise and write the fp32 NCHW batch the backbone reads, in ONE launch per batch (`contrast` needs
// the integer plane sums of rovit_corrupt_stats first).  The specification of record is rovit_hip/corrupt.py's docstring;
// corrupt_reference there is the numpy restatement the tests compare against.  The output has the store's own resolution.
//
// Four kernel shapes:
//   pointwise  gaussian_noise, shot_noise, impulse_noise, brightness, contrast, saturate.  A lane owns 4 consecutive pixels of a row in all
//              three planes (one uchar4 load and one float4 store per plane when the width is a multiple of 4, element accesses otherwise).
//   cell       pixelate: the same ownership; a pixel reads its b x b cell (clipped at the image edge) and takes the integer sum.
//   stencil    gaussian_blur, defocus_blur, motion_blur.  A workgroup owns a 32 x 64 tile of ONE plane: the uint8 tile with its halo
//              (edge-replicated: the coordinates are clamped when the tile is staged) goes to LDS once, the per-image weight / offset table
//              is built in LDS at workgroup start, a lane computes 8 consecutive pixels of a row.  The Gaussian is separable (a horizontal
//              pass into an fp32 LDS tile, then a vertical one); the disk is a sliding integer row sum per dy; the motion blur's bilinear
//              samples share ONE fractional offset per k (x + k cos(theta) = x + floor(.) + frac(.) with x an integer), so its table
//              holds an integer offset and four weights per k and the taps are exact uint8 reads.
//   8x8 codec  jpeg: a wave owns one 8 x 8 block of all three planes (the colour conversion couples them); both passes of the forward and
//              of the inverse transform go through LDS; integers end to end.
//
// Every draw is Philox4x32-10 (philox.h) keyed by the image's index in the STORE and the pixel's index in the image, a pixel's arithmetic depends on
// nothing else, and the only cross-thread reduction (the plane sums of `contrast`) is an integer sum: a corrupted image has the same
// bits for every batch size, order and split, and from run to run.  There is no floating-point atomic in this file.
//
// A store index outside [0, n_images) is never dereferenced: the sample's output is NaN (its out_u8 rows and plane sums are 0).
#include <math.h>

#include "common.h"
#include "philox.h"

namespace {

constexpr int CB_NT = 256;
constexpr int CB_HALO = ROVIT_CORRUPT_MAX_RADIUS;        // 18: gaussian sigma = 6 (R = 18), motion R = 17 (R + 1 taps), disk r = 18
constexpr int ST_TW = 64, ST_TH = 32;                    // stencil tile: 32 rows of 64 pixels, 8 pixels per lane
constexpr int ST_PW = ST_TW + 2 * CB_HALO, ST_PH = ST_TH + 2 * CB_HALO;
constexpr int ST_TAPS = 2 * CB_HALO + 1;

constexpr float TWO_PI = 6.283185307179586f;

struct CorArgs {
  const unsigned char* src; const long long* indices; const long long* sums; float* out; unsigned char* out_u8;
  unsigned long long seed;
  float p;
  int kind, N, H, W, chunks, vec;          // vec: W % 4 == 0 and src / out / out_u8 aligned for 4-byte loads and 16-byte stores
};

__device__ __forceinline__ float clamp01(float z) { return fminf(fmaxf(z, 0.f), 1.f); }
__device__ __forceinline__ float norm_c(float z, int c) {
  return c == 0 ? fmaf(z, (float)(1.0 / 0.229), -(float)(0.485 / 0.229))
       : c == 1 ? fmaf(z, (float)(1.0 / 0.224), -(float)(0.456 / 0.224))
                : fmaf(z, (float)(1.0 / 0.225), -(float)(0.406 / 0.225));
}
__device__ __forceinline__ unsigned char quant_u8(float z) { return (unsigned char)floorf(fmaf(255.f, z, 0.5f)); }

// nx (<= 4) consecutive pixels of one plane row: z already clamped to [0, 1]
__device__ __forceinline__ void store_row4(const CorArgs& a, size_t plane_off, int c, const float z[4], int nx) {
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = norm_c(z[e], c);
  if (a.vec) {
    *reinterpret_cast<float4*>(a.out + plane_off) = make_float4(o[0], o[1], o[2], o[3]);
    if (a.out_u8) *reinterpret_cast<uchar4*>(a.out_u8 + plane_off) = make_uchar4(quant_u8(z[0]), quant_u8(z[1]), quant_u8(z[2]), quant_u8(z[3]));
  } else {
    for (int e = 0; e < nx; ++e) {
      a.out[plane_off + e] = o[e];
      if (a.out_u8) a.out_u8[plane_off + e] = quant_u8(z[e]);
    }
  }
}

// NaN sample: every lane of the workgroups that serve sample n fills its share
__device__ void fill_bad(const CorArgs& a, int n, int part, int parts) {
  const size_t total = (size_t)3 * a.H * a.W;
  const float q = __builtin_nanf("");
  for (size_t i = (size_t)part * CB_NT + threadIdx.x; i < total; i += (size_t)parts * CB_NT) {
    a.out[(size_t)n * total + i] = q;
    if (a.out_u8) a.out_u8[(size_t)n * total + i] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// pointwise
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_NT) void corrupt_point_kernel(const CorArgs a) {
  __shared__ float sh_mean[3];
  const int n = blockIdx.x / a.chunks, chunk = blockIdx.x - n * a.chunks;
  const long long image = a.indices[n];
  if (image < 0 || image >= a.N) { fill_bad(a, n, chunk, a.chunks); return; }
  const size_t plane = (size_t)a.H * a.W;
  if (a.kind == ROVIT_CORRUPT_CONTRAST) {
    if (threadIdx.x < 3) sh_mean[threadIdx.x] = (float)((double)a.sums[(size_t)n * 3 + threadIdx.x] / (255.0 * (double)plane));
    __syncthreads();
  }
  const unsigned char* const src = a.src + (size_t)image * 3 * plane;
  const int W4 = (a.W + 3) >> 2, items = a.H * W4;
  const int kind = a.kind;
  const float p = a.p;
  const float imp_lo = 0.5f * p, imp_hi = 1.0f - imp_lo;
  float mean[3] = {0.f, 0.f, 0.f};
  if (kind == ROVIT_CORRUPT_CONTRAST) { mean[0] = sh_mean[0]; mean[1] = sh_mean[1]; mean[2] = sh_mean[2]; }

  for (int it = chunk * CB_NT + threadIdx.x; it < items; it += a.chunks * CB_NT) {
    const int y = it / W4, x0 = (it - y * W4) << 2;
    const int nx = min(4, a.W - x0);
    const size_t off = (size_t)y * a.W + x0;
    float v[3][4];
    if (a.vec) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uchar4 q = *reinterpret_cast<const uchar4*>(src + c * plane + off);
        v[c][0] = (float)q.x; v[c][1] = (float)q.y; v[c][2] = (float)q.z; v[c][3] = (float)q.w;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[c][e] = e < nx ? (float)src[c * plane + off + e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float r = v[0][e] * (1.0f / 255.0f), g = v[1][e] * (1.0f / 255.0f), b = v[2][e] * (1.0f / 255.0f);
      if (kind == ROVIT_CORRUPT_GAUSSIAN_NOISE || kind == ROVIT_CORRUPT_SHOT_NOISE) {
        const U4 w = philox4x32_10(a.seed, (unsigned)(off + e), (unsigned)image, (unsigned)kind, 0u);
        const float r0 = sqrtf(-2.0f * logf(u01_open(w.x))), r1 = sqrtf(-2.0f * logf(u01_open(w.z)));
        float sn, cs;
        sincosf(TWO_PI * u01(w.y), &sn, &cs);
        const float n0 = r0 * cs, n1 = r0 * sn, n2 = r1 * cosf(TWO_PI * u01(w.w));
        if (kind == ROVIT_CORRUPT_GAUSSIAN_NOISE) {
          r = fmaf(p, n0, r); g = fmaf(p, n1, g); b = fmaf(p, n2, b);
        } else {
          r = fmaf(sqrtf(r / p), n0, r); g = fmaf(sqrtf(g / p), n1, g); b = fmaf(sqrtf(b / p), n2, b);
        }
      } else if (kind == ROVIT_CORRUPT_IMPULSE_NOISE) {
        const U4 w = philox4x32_10(a.seed, (unsigned)(off + e), (unsigned)image, (unsigned)kind, 0u);
        const float u0 = u01(w.x), u1 = u01(w.y), u2 = u01(w.z);
        r = u0 < imp_lo ? 0.f : (u0 >= imp_hi ? 1.f : r);
        g = u1 < imp_lo ? 0.f : (u1 >= imp_hi ? 1.f : g);
        b = u2 < imp_lo ? 0.f : (u2 >= imp_hi ? 1.f : b);
      } else if (kind == ROVIT_CORRUPT_BRIGHTNESS) {
        r += p; g += p; b += p;
      } else if (kind == ROVIT_CORRUPT_CONTRAST) {
        const float q = 1.0f - p;                                   // m + c (v - m) = v + (1 - c) (m - v): exactly v at c = 1
        r = fmaf(q, mean[0] - r, r); g = fmaf(q, mean[1] - g, g); b = fmaf(q, mean[2] - b, b);
      } else {                                                      // saturate
        const float grey = fmaf(0.299f, r, fmaf(0.587f, g, 0.114f * b)), q = 1.0f - p;
        r = fmaf(q, grey - r, r); g = fmaf(q, grey - g, g); b = fmaf(q, grey - b, b);
      }
      v[0][e] = clamp01(r); v[1][e] = clamp01(g); v[2][e] = clamp01(b);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) store_row4(a, ((size_t)n * 3 + c) * plane + off, c, v[c], nx);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// cell (pixelate): a.p carries the cell side b as an integer value
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_NT) void corrupt_cell_kernel(const CorArgs a) {
  const int n = blockIdx.x / a.chunks, chunk = blockIdx.x - n * a.chunks;
  const long long image = a.indices[n];
  if (image < 0 || image >= a.N) { fill_bad(a, n, chunk, a.chunks); return; }
  const size_t plane = (size_t)a.H * a.W;
  const unsigned char* const src = a.src + (size_t)image * 3 * plane;
  const int W4 = (a.W + 3) >> 2, items = a.H * W4;
  const int b = (int)a.p;
  for (int it = chunk * CB_NT + threadIdx.x; it < items; it += a.chunks * CB_NT) {
    const int y = it / W4, x0 = (it - y * W4) << 2;
    const int nx = min(4, a.W - x0);
    const size_t off = (size_t)y * a.W + x0;
    const int cy0 = (y / b) * b, cy1 = min(cy0 + b, a.H);
    float z[3][4];
    int last_cell = -1;
    float zc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = min(x0 + e, a.W - 1), cell = x / b;
      if (cell != last_cell) {
        last_cell = cell;
        const int cx0 = cell * b, cx1 = min(cx0 + b, a.W);
        const float denom = 255.0f * (float)((cy1 - cy0) * (cx1 - cx0));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          int s = 0;
          for (int yy = cy0; yy < cy1; ++yy)
            for (int xx = cx0; xx < cx1; ++xx) s += src[c * plane + (size_t)yy * a.W + xx];
          zc[c] = clamp01((float)s / denom);
        }
      }
      z[0][e] = zc[0]; z[1][e] = zc[1]; z[2][e] = zc[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) store_row4(a, ((size_t)n * 3 + c) * plane + off, c, z[c], nx);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// stencil
// ---------------------------------------------------------------------------------------------------------------------------------
struct StencilArgs {
  CorArgs a;
  int R, halo, tiles_x, tiles_y;
  float weights[CB_HALO + 1];             // gaussian: normalised 1-D weights of |k| = 0..R (host, fp64 rounded once)
  unsigned char spans[CB_HALO + 1];       // disk: largest s with s^2 + dy^2 <= r^2, for |dy| = 0..R (host, fp64)
  float inv_count;                        // disk: 1 / (255 count)
};

struct MotionTap { int ox, oy; float w00, w01, w10, w11; };

__global__ __launch_bounds__(CB_NT) void corrupt_stencil_kernel(const StencilArgs s) {
  __shared__ unsigned char tile[ST_PH][ST_PW + 4];
  __shared__ float inter[ST_PH][ST_TW];
  __shared__ float sh_w[CB_HALO + 1];
  __shared__ int sh_span[CB_HALO + 1];
  __shared__ MotionTap sh_tap[ST_TAPS];
  const CorArgs& a = s.a;
  const int per_image = 3 * s.tiles_x * s.tiles_y;
  const int n = blockIdx.x / per_image, rem = blockIdx.x - n * per_image;
  const long long image = a.indices[n];
  if (image < 0 || image >= a.N) { fill_bad(a, n, rem, per_image); return; }
  const int c = rem / (s.tiles_x * s.tiles_y), t = rem - c * (s.tiles_x * s.tiles_y);
  const int ty0 = (t / s.tiles_x) * ST_TH, tx0 = (t % s.tiles_x) * ST_TW;
  const size_t plane = (size_t)a.H * a.W;
  const unsigned char* const src = a.src + ((size_t)image * 3 + c) * plane;
  const int R = s.R, halo = s.halo, kind = a.kind;

  // the table
  if (threadIdx.x <= R) {
    sh_w[threadIdx.x] = s.weights[threadIdx.x];
    sh_span[threadIdx.x] = s.spans[threadIdx.x];
  }
  if (kind == ROVIT_CORRUPT_MOTION_BLUR && threadIdx.x < 2 * R + 1) {
    const U4 w = philox4x32_10(a.seed, (unsigned)image, 0u, (unsigned)kind, 1u);
    float sn, cs;
    sincosf(TWO_PI * u01(w.x), &sn, &cs);
    const float k = (float)((int)threadIdx.x - R);
    const float dx = k * cs, dy = k * sn;
    const float ix = floorf(dx), iy = floorf(dy);
    const float fx = dx - ix, fy = dy - iy;
    MotionTap m;
    m.ox = (int)ix; m.oy = (int)iy;
    m.w00 = (1.f - fx) * (1.f - fy); m.w01 = fx * (1.f - fy); m.w10 = (1.f - fx) * fy; m.w11 = fx * fy;
    sh_tap[threadIdx.x] = m;
  }
  // the tile and its halo: coordinates clamped to the image = edges replicate
  const int th = ST_TH + 2 * halo, tw = ST_TW + 2 * halo;
  for (int i = threadIdx.x; i < th * tw; i += CB_NT) {
    const int r = i / tw, q = i - r * tw;
    const int gy = min(max(ty0 - halo + r, 0), a.H - 1), gx = min(max(tx0 - halo + q, 0), a.W - 1);
    tile[r][q] = src[(size_t)gy * a.W + gx];
  }
  __syncthreads();

  const int row = threadIdx.x >> 3, xg = (threadIdx.x & 7) << 3;       // 8 consecutive pixels of tile row `row`
  float z[8];
  if (kind == ROVIT_CORRUPT_GAUSSIAN_BLUR) {
    for (int i = threadIdx.x; i < th * ST_TW; i += CB_NT) {
      const int r = i >> 6, q = i & (ST_TW - 1);
      float acc = sh_w[0] * (float)tile[r][q + halo];
      for (int k = 1; k <= R; ++k) acc = fmaf(sh_w[k], (float)tile[r][q + halo - k] + (float)tile[r][q + halo + k], acc);
      inter[r][q] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float acc = sh_w[0] * inter[row + halo][xg + e];
      for (int k = 1; k <= R; ++k) acc = fmaf(sh_w[k], inter[row + halo - k][xg + e] + inter[row + halo + k][xg + e], acc);
      z[e] = clamp01(acc * (1.0f / 255.0f));
    }
  } else if (kind == ROVIT_CORRUPT_DEFOCUS_BLUR) {
    int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int dy = -R; dy <= R; ++dy) {
      const int sp = sh_span[dy < 0 ? -dy : dy];
      const unsigned char* const line = &tile[row + halo + dy][xg + halo];
      int sum = 0;
      for (int dx = -sp; dx <= sp; ++dx) sum += line[dx];
      acc[0] += sum;
#pragma unroll
      for (int e = 1; e < 8; ++e) {
        sum += (int)line[e + sp] - (int)line[e - 1 - sp];
        acc[e] += sum;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = clamp01((float)acc[e] * s.inv_count);
  } else {                                                             // motion blur
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 2 * R + 1; ++k) {
      const MotionTap m = sh_tap[k];
      const unsigned char* const l0 = &tile[row + halo + m.oy][xg + halo + m.ox];
      const unsigned char* const l1 = &tile[row + halo + m.oy + 1][xg + halo + m.ox];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        acc[e] += fmaf(m.w00, (float)l0[e], fmaf(m.w01, (float)l0[e + 1], fmaf(m.w10, (float)l1[e], m.w11 * (float)l1[e + 1])));
    }
    const float sc = 1.0f / (255.0f * (float)(2 * R + 1));
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = clamp01(acc[e] * sc);
  }

  const int gy = ty0 + row, gx = tx0 + xg;
  if (gy >= a.H || gx >= a.W) return;
  const size_t off = ((size_t)n * 3 + c) * plane + (size_t)gy * a.W + gx;
  store_row4(a, off, c, z, min(4, a.W - gx));
  if (gx + 4 < a.W) store_row4(a, off + 4, c, z + 4, min(4, a.W - gx - 4));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// jpeg
// ---------------------------------------------------------------------------------------------------------------------------------
struct JpegArgs {
  CorArgs a;
  int blocks_x, blocks_y, groups;         // 8 x 8 blocks per image; workgroups per image (4 blocks each)
  int M[64];                              // M[u][x] = rint(8192 a(u) cos((2x + 1) u pi / 16))
  int Q[2][64];                           // scaled luminance and chrominance tables
};

__global__ __launch_bounds__(CB_NT) void corrupt_jpeg_kernel(const JpegArgs j) {
  __shared__ int sh_m[64], sh_q[2][64];
  __shared__ int A[4][3][64], B[4][3][64];
  const CorArgs& a = j.a;
  const int n = blockIdx.x / j.groups, grp = blockIdx.x - n * j.groups;
  const long long image = a.indices[n];
  if (image < 0 || image >= a.N) { fill_bad(a, n, grp, j.groups); return; }
  if (threadIdx.x < 64) sh_m[threadIdx.x] = j.M[threadIdx.x];
  else if (threadIdx.x < 192) (&sh_q[0][0])[threadIdx.x - 64] = (&j.Q[0][0])[threadIdx.x - 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane >> 3, q = lane & 7;
  const int nblk = j.blocks_x * j.blocks_y;
  const int blk_raw = grp * 4 + wave;
  const bool live = blk_raw < nblk;
  const int blk = live ? blk_raw : nblk - 1;                            // an idle wave redoes the last block and stores nothing
  const int by = blk / j.blocks_x, bx = blk - by * j.blocks_x;
  const int py = by * 8 + r, px = bx * 8 + q;
  const size_t plane = (size_t)a.H * a.W;
  const unsigned char* const src = a.src + (size_t)image * 3 * plane;
  const size_t soff = (size_t)min(py, a.H - 1) * a.W + min(px, a.W - 1);   // sides that are no multiple of 8: edge-replicated
  {
    const int Rr = src[soff], Gg = src[plane + soff], Bb = src[2 * plane + soff];
    A[wave][0][lane] = ((19595 * Rr + 38470 * Gg + 7471 * Bb + 32768) >> 16) - 128;
    A[wave][1][lane] = ((-11059 * Rr - 21709 * Gg + 32768 * Bb + (128 << 16) + 32767) >> 16) - 128;
    A[wave][2][lane] = ((32768 * Rr - 27439 * Gg - 5329 * Bb + (128 << 16) + 32767) >> 16) - 128;
  }
  __syncthreads();
  // forward, along y: t[u][x] = sum_y M[u][y] blk[y][x]   (u = r, x = q)
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    int t = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += sh_m[r * 8 + k] * A[wave][p][k * 8 + q];
    B[wave][p][lane] = (t + 512) >> 10;
  }
  __syncthreads();
  // forward, along x: c[u][v] = sum_x t[u][x] M[v][x]   (u = r, v = q); quantise, dequantise
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) c += B[wave][p][r * 8 + k] * sh_m[q * 8 + k];
    const int Q = sh_q[p ? 1 : 0][lane];
    const int mag = ((c < 0 ? -c : c) + (Q << 15)) / (Q << 16);
    A[wave][p][lane] = (c < 0 ? -mag : mag) * Q;
  }
  __syncthreads();
  // inverse, along u: w[y][v] = sum_u M[u][y] d[u][v]   (y = r, v = q)
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    int w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w += sh_m[k * 8 + r] * A[wave][p][k * 8 + q];
    B[wave][p][lane] = (w + 512) >> 10;
  }
  __syncthreads();
  // inverse, along v: r[y][x] = sum_v w[y][v] M[v][x]   (y = r, x = q)
  int lev[3];
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += B[wave][p][r * 8 + k] * sh_m[k * 8 + q];
    lev[p] = min(max(((s + 32768) >> 16) + 128, 0), 255);
  }
  if (!live || py >= a.H || px >= a.W) return;
  const int cb = lev[1] - 128, cr = lev[2] - 128;
  int rgb[3];
  rgb[0] = lev[0] + ((91881 * cr + 32768) >> 16);
  rgb[1] = lev[0] + ((-22554 * cb - 46802 * cr + 32768) >> 16);
  rgb[2] = lev[0] + ((116130 * cb + 32768) >> 16);
  const size_t off = (size_t)py * a.W + px;
  const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const int level = min(max(rgb[p], 0), 255);
    // 256 possible values per plane: fp64 and one rounding, so that the fp32 output is the nearest fp32 to the reference's fp64
    a.out[((size_t)n * 3 + p) * plane + off] = (float)(((double)level / 255.0 - mean[p]) / sd[p]);
    if (a.out_u8) a.out_u8[((size_t)n * 3 + p) * plane + off] = (unsigned char)level;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plane sums (contrast): one workgroup per (sample, plane), integer tree in a fixed order
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_NT) void corrupt_stats_kernel(const unsigned char* src, const long long* indices, long long* sums, int N,
                                                              int H, int W) {
  __shared__ unsigned long long part[CB_NT];
  const int n = blockIdx.x / 3, c = blockIdx.x - n * 3;
  const long long image = indices[n];
  if (image < 0 || image >= N) {
    if (threadIdx.x == 0) sums[(size_t)n * 3 + c] = 0;
    return;
  }
  const size_t plane = (size_t)H * W;
  const unsigned char* const p = src + ((size_t)image * 3 + c) * plane;
  unsigned long long acc = 0;
  if ((((uintptr_t)p) & 3u) == 0) {
    const size_t words = plane >> 2;
    const unsigned* const pw = reinterpret_cast<const unsigned*>(p);
    for (size_t i = threadIdx.x; i < words; i += CB_NT) {
      const unsigned w = pw[i];
      acc += (w & 0xFFu) + ((w >> 8) & 0xFFu) + ((w >> 16) & 0xFFu) + (w >> 24);
    }
    for (size_t i = (words << 2) + threadIdx.x; i < plane; i += CB_NT) acc += p[i];
  } else {
    for (size_t i = threadIdx.x; i < plane; i += CB_NT) acc += p[i];
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = CB_NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[(size_t)n * 3 + c] = (long long)part[0];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
const int JPEG_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                           14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const int JPEG_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                             47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

int check_common(const char* what, const unsigned char* src, int n_images, int h, int w, const long long* indices, int batch) {
  ROVIT_CHECK_ARG(src && indices, ROVIT_ERR_NULL, "%s: null pointer (src, indices)", what);
  ROVIT_CHECK_ARG(n_images > 0 && h >= 8 && w >= 8, ROVIT_ERR_SHAPE, "%s: store of %d images of %d x %d (sides must be >= 8)", what, n_images,
                  h, w);
  ROVIT_CHECK_ARG((size_t)h * w <= (size_t)1 << 28, ROVIT_ERR_SHAPE, "%s: image plane too large", what);
  ROVIT_CHECK_ARG(batch > 0, ROVIT_ERR_SHAPE, "%s: empty batch", what);
  return ROVIT_OK;
}

}  // namespace

extern "C" int rovit_corrupt_stats(const unsigned char* src, int n_images, int src_h, int src_w, const long long* indices, int batch,
                                   long long* sums, rovit_stream_t stream) {
  const int rc = check_common("corrupt_stats", src, n_images, src_h, src_w, indices, batch);
  if (rc != ROVIT_OK) return rc;
  ROVIT_CHECK_ARG(sums, ROVIT_ERR_NULL, "corrupt_stats: null pointer (sums)");
  ROVIT_CHECK_ARG((size_t)batch * 3 < (size_t)1 << 31, ROVIT_ERR_SHAPE, "corrupt_stats: batch %d too large for one launch", batch);
  hipLaunchKernelGGL(corrupt_stats_kernel, dim3((unsigned)batch * 3u), dim3(CB_NT), 0, (hipStream_t)stream, src, indices, sums, n_images,
                     src_h, src_w);
  ROVIT_CHECK_LAUNCH("corrupt_stats_kernel");
  return ROVIT_OK;
}

extern "C" int rovit_corrupt_batch(const unsigned char* src, int n_images, int src_h, int src_w, const long long* indices, int batch,
                                   const rovit_corruption* desc, const long long* sums, float* out, unsigned char* out_u8,
                                   rovit_stream_t stream) {
  const int rc = check_common("corrupt_batch", src, n_images, src_h, src_w, indices, batch);
  if (rc != ROVIT_OK) return rc;
  ROVIT_CHECK_ARG(desc && out, ROVIT_ERR_NULL, "corrupt_batch: null pointer (desc, out)");
  const int kind = desc->kind;
  const float p = desc->param;
  ROVIT_CHECK_ARG(kind >= 0 && kind < ROVIT_CORRUPT_COUNT, ROVIT_ERR_SHAPE, "corrupt_batch: unknown corruption id %d", kind);
  ROVIT_CHECK_ARG(isfinite(p), ROVIT_ERR_SHAPE, "corrupt_batch: parameter %g is not finite", p);
  ROVIT_CHECK_ARG(kind != ROVIT_CORRUPT_CONTRAST || sums, ROVIT_ERR_NULL, "corrupt_batch: contrast needs the plane sums of rovit_corrupt_stats");
  const size_t plane = (size_t)src_h * src_w;
  const size_t src_bytes = (size_t)n_images * 3 * plane, out_elems = (size_t)batch * 3 * plane;
  const uintptr_t s0 = (uintptr_t)src, o0 = (uintptr_t)out, q0 = (uintptr_t)out_u8;
  ROVIT_CHECK_ARG(s0 + src_bytes <= o0 || o0 + out_elems * sizeof(float) <= s0, ROVIT_ERR_SHAPE, "corrupt_batch: out aliases src");
  ROVIT_CHECK_ARG(!out_u8 || s0 + src_bytes <= q0 || q0 + out_elems <= s0, ROVIT_ERR_SHAPE, "corrupt_batch: out_u8 aliases src");
  ROVIT_CHECK_ARG(((uintptr_t)out & 3u) == 0, ROVIT_ERR_ALIGN, "corrupt_batch: out must be 4-byte aligned");

  CorArgs a{};
  a.src = src; a.indices = indices; a.sums = sums; a.out = out; a.out_u8 = out_u8;
  a.seed = desc->seed; a.p = p; a.kind = kind; a.N = n_images; a.H = src_h; a.W = src_w;
  a.vec = src_w % 4 == 0 && (s0 & 3u) == 0 && rovit_aligned16(out) && (q0 & 3u) == 0;
  // workgroups per sample of the pointwise and cell kernels: as in augment_batch
  const size_t items = (size_t)src_h * ((src_w + 3) / 4);
  const size_t max_chunks = (items + CB_NT - 1) / CB_NT;
  size_t chunks = (size_t)(2048 + batch - 1) / batch;
  const size_t by_work = (items + 8 * CB_NT - 1) / (8 * CB_NT);
  if (chunks < by_work) chunks = by_work;
  if (chunks > max_chunks) chunks = max_chunks;
  a.chunks = (int)chunks;
  const size_t limit = (size_t)1 << 31;

  switch (kind) {
    case ROVIT_CORRUPT_GAUSSIAN_NOISE:
    case ROVIT_CORRUPT_SHOT_NOISE:
    case ROVIT_CORRUPT_IMPULSE_NOISE:
    case ROVIT_CORRUPT_BRIGHTNESS:
    case ROVIT_CORRUPT_CONTRAST:
    case ROVIT_CORRUPT_SATURATE: {
      ROVIT_CHECK_ARG(kind != ROVIT_CORRUPT_GAUSSIAN_NOISE || p >= 0.f, ROVIT_ERR_SHAPE, "corrupt_batch: gaussian_noise sigma %g < 0", p);
      ROVIT_CHECK_ARG(kind != ROVIT_CORRUPT_SHOT_NOISE || p > 0.f, ROVIT_ERR_SHAPE, "corrupt_batch: shot_noise c = %g must be > 0", p);
      ROVIT_CHECK_ARG(kind != ROVIT_CORRUPT_IMPULSE_NOISE || (p >= 0.f && p <= 1.f), ROVIT_ERR_SHAPE,
                      "corrupt_batch: impulse_noise p = %g outside [0, 1]", p);
      ROVIT_CHECK_ARG((size_t)batch * chunks < limit, ROVIT_ERR_SHAPE, "corrupt_batch: batch %d too large for one launch", batch);
      hipLaunchKernelGGL(corrupt_point_kernel, dim3((unsigned)((size_t)batch * chunks)), dim3(CB_NT), 0, (hipStream_t)stream, a);
      ROVIT_CHECK_LAUNCH("corrupt_point_kernel");
      return ROVIT_OK;
    }
    case ROVIT_CORRUPT_PIXELATE: {
      ROVIT_CHECK_ARG(p >= 1.f && p <= 64.f && p == floorf(p), ROVIT_ERR_SHAPE, "corrupt_batch: pixelate cell side %g must be an integer in 1..64",
                      p);
      ROVIT_CHECK_ARG((size_t)batch * chunks < limit, ROVIT_ERR_SHAPE, "corrupt_batch: batch %d too large for one launch", batch);
      hipLaunchKernelGGL(corrupt_cell_kernel, dim3((unsigned)((size_t)batch * chunks)), dim3(CB_NT), 0, (hipStream_t)stream, a);
      ROVIT_CHECK_LAUNCH("corrupt_cell_kernel");
      return ROVIT_OK;
    }
    case ROVIT_CORRUPT_GAUSSIAN_BLUR:
    case ROVIT_CORRUPT_DEFOCUS_BLUR:
    case ROVIT_CORRUPT_MOTION_BLUR: {
      StencilArgs s{};
      s.a = a;
      if (kind == ROVIT_CORRUPT_GAUSSIAN_BLUR) {
        ROVIT_CHECK_ARG(p > 0.f && ceil(3.0 * (double)p) <= CB_HALO, ROVIT_ERR_SHAPE,
                        "corrupt_batch: gaussian_blur sigma %g must satisfy 0 < sigma and ceil(3 sigma) <= %d", p, CB_HALO);
        s.R = (int)ceil(3.0 * (double)p);
        s.halo = s.R;
        double w[CB_HALO + 1], total = 0.0;
        for (int k = 0; k <= s.R; ++k) {
          w[k] = exp(-(double)(k * k) / (2.0 * (double)p * (double)p));
          total += k ? 2.0 * w[k] : w[k];
        }
        for (int k = 0; k <= s.R; ++k) s.weights[k] = (float)(w[k] / total);
      } else if (kind == ROVIT_CORRUPT_DEFOCUS_BLUR) {
        ROVIT_CHECK_ARG(p >= 0.f && p <= (float)CB_HALO, ROVIT_ERR_SHAPE, "corrupt_batch: defocus_blur radius %g outside [0, %d]", p, CB_HALO);
        s.R = (int)floor((double)p);
        s.halo = s.R;
        const double r2 = (double)p * (double)p;
        long long count = 0;
        for (int dy = 0; dy <= s.R; ++dy) {
          int sp = 0;
          while ((double)((sp + 1) * (sp + 1) + dy * dy) <= r2) ++sp;
          s.spans[dy] = (unsigned char)sp;
          count += (dy ? 2 : 1) * (2 * sp + 1);
        }
        s.inv_count = (float)(1.0 / (255.0 * (double)count));
      } else {
        ROVIT_CHECK_ARG(p >= 0.f && p <= (float)(CB_HALO - 1) && p == floorf(p), ROVIT_ERR_SHAPE,
                        "corrupt_batch: motion_blur half-length %g must be an integer in 0..%d", p, CB_HALO - 1);
        s.R = (int)p;
        s.halo = s.R + 1;
      }
      s.tiles_x = (src_w + ST_TW - 1) / ST_TW;
      s.tiles_y = (src_h + ST_TH - 1) / ST_TH;
      const size_t grid = (size_t)batch * 3 * s.tiles_x * s.tiles_y;
      ROVIT_CHECK_ARG(grid < limit, ROVIT_ERR_SHAPE, "corrupt_batch: batch %d too large for one launch", batch);
      hipLaunchKernelGGL(corrupt_stencil_kernel, dim3((unsigned)grid), dim3(CB_NT), 0, (hipStream_t)stream, s);
      ROVIT_CHECK_LAUNCH("corrupt_stencil_kernel");
      return ROVIT_OK;
    }
    default: {                                                          // jpeg
      ROVIT_CHECK_ARG(p >= 1.f && p <= 100.f && p == floorf(p), ROVIT_ERR_SHAPE, "corrupt_batch: jpeg quality %g must be an integer in 1..100", p);
      JpegArgs j{};
      j.a = a;
      const int quality = (int)p;
      const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
      for (int k = 0; k < 64; ++k) {
        const int l = (JPEG_LUMA[k] * scale + 50) / 100, c = (JPEG_CHROMA[k] * scale + 50) / 100;
        j.Q[0][k] = l < 1 ? 1 : (l > 255 ? 255 : l);
        j.Q[1][k] = c < 1 ? 1 : (c > 255 ? 255 : c);
      }
      for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x)
          j.M[u * 8 + x] = (int)rint(8192.0 * (u ? 0.5 : sqrt(0.125)) * cos((double)((2 * x + 1) * u) * 3.14159265358979323846 / 16.0));
      j.blocks_x = (src_w + 7) / 8;
      j.blocks_y = (src_h + 7) / 8;
      j.groups = (j.blocks_x * j.blocks_y + 3) / 4;
      const size_t grid = (size_t)batch * j.groups;
      ROVIT_CHECK_ARG(grid < limit, ROVIT_ERR_SHAPE, "corrupt_batch: batch %d too large for one launch", batch);
      hipLaunchKernelGGL(corrupt_jpeg_kernel, dim3((unsigned)grid), dim3(CB_NT), 0, (hipStream_t)stream, j);
      ROVIT_CHECK_LAUNCH("corrupt_jpeg_kernel");
      return ROVIT_OK;
    }
  }
}
