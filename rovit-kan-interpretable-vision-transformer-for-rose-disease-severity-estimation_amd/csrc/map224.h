// The 14x14 -> 224x224 bilinear resize shared by the explainability map kernels (rollout.hip, gradcam.hip): what the
// reference's cv2.resize(INTER_LINEAR) does to a float patch grid, i.e. F.interpolate(mode='bilinear', align_corners=False):
// half-pixel centres, source coordinates clamped at 0, the right / bottom neighbour clamped at the last row / column.
#pragma once
#include "common.h"

static constexpr int GRID = 14, MAP = 224;

// output pixel (y, x) of the resized 14x14 grid g
static __device__ __forceinline__ float bilinear14(const float* g, int y, int x) {
  const float sc = (float)GRID / MAP;
  const float sy = fmaxf(sc * (y + 0.5f) - 0.5f, 0.f), sx = fmaxf(sc * (x + 0.5f) - 0.5f, 0.f);
  const int y0 = (int)sy, x0 = (int)sx;
  const int yp = y0 < GRID - 1 ? 1 : 0, xp = x0 < GRID - 1 ? 1 : 0;
  const float ly1 = sy - y0, ly0 = 1.f - ly1, lx1 = sx - x0, lx0 = 1.f - lx1;
  const float* r0 = g + y0 * GRID + x0;
  const float* r1 = r0 + yp * GRID;
  return ly0 * (lx0 * r0[0] + lx1 * r0[xp]) + ly1 * (lx0 * r1[0] + lx1 * r1[xp]);
}
