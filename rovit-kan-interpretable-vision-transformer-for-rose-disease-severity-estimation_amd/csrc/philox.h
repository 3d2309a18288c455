// Philox4x32-10 (Salmon et al., SC 2011): the library's only device random generator, and the device twin of oracle/philox.py.
// key = the 64-bit seed, counter = four 32-bit words, ten rounds; every draw is a pure function of (seed, counter), so a
// result never depends on the grid, the batch split or the order of the launches.
//
// Who uses which counter -- the streams have to stay disjoint for one seed, and this list is where to check that:
//   head-phase dropout masks   head_phase.hip      (b * hid + k, 0, offset lo, offset hi)       words x / y / z -> heads 0 / 1 / 2
//   MC dropout                 mc_dropout.hip      (b * hid + k, t, offset lo, offset hi)       sample t = 0 is the head phase's draw
//   augmentation               augment_batch.hip   (image, row 0..2, epoch lo, epoch hi)
//   corruptions                corrupt.hip         (pixel, image, kind, 0) a pixel's draw; (image, 0, kind, 1) the per-image draw
//   bootstrap resamples        eval_bootstrap.hip  (q, r, ROVIT_EVAL_BOOT_STREAM, 0)
//   conformal randomisation    conformal_device.h  (row, 0, ROVIT_EVAL_CONF_STREAM, 0)
//   KernelSHAP coalitions      shap.hip            (player / 4, sampled pair r, ROVIT_SHAP_STREAM, 0)  word player % 4 is the player's key
//   PatchDropout subsets       patch_dropout.hip   (sample b, ROVIT_PATCH_DROPOUT_STREAM + patch / 4, step lo, step hi)  word patch % 4 is the patch's key
//   k-means++ seeding          kmeans.hip          (seed index j, restart r, ROVIT_KMEANS_STREAM, 0)  r64 = (x << 32) | y
//   PGD random start           attack.hip          (element / 4, image id, ROVIT_ATTACK_STREAM, restart)  word element % 4 is the element's
// A caller with a 64-bit offset splits it at the call: (unsigned)off, (unsigned)(off >> 32).
#pragma once
#include <hip/hip_runtime.h>

struct U4 { unsigned x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  U4 c = {c0, c1, c2, c3};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c;
}

// the top 24 bits of a word as a uniform fp32 (every value is exact)
__device__ __forceinline__ float u01(unsigned x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }            // [0, 1)
__device__ __forceinline__ float u01_open(unsigned x) { return (float)((x >> 8) + 1u) * (1.0f / 16777216.0f); }  // (0, 1]
