// The unit-cost edit distance of two symbol sequences by one workgroup: the core under the corpus evaluator (wer.hip) and the
// validation error rates (editdist.hip).  Integer arithmetic only; the lattice never leaves the three LDS diagonals.
#pragma once
#include "common.h"

namespace tavsr {

// D[i][j]: i symbols of r against j symbols of h; anti-diagonal k holds D[i][k - i] at index i.  `diag`: 3 * stride LDS words,
// stride >= Lr + 1.  Every thread of the block calls it (it synchronises) and every thread receives D[Lr][Lh].  r / h may point
// to global memory or to LDS; r[0 .. Lr) and h[0 .. Lh) are all that is read.  The caller synchronises before it reuses `diag`.
__device__ __forceinline__ int edit_distance_core(const int32_t* r, int Lr, const int32_t* h, int Lh, int32_t* diag, int stride) {
  int a = 0, b = stride, c = 2 * stride;             // diagonals k - 2, k - 1, k
  if (threadIdx.x == 0) diag[b] = 0;                 // k = 0: D[0][0]
  __syncthreads();
  for (int k = 1; k <= Lr + Lh; ++k) {
    const int lo = max(0, k - Lh), hi = min(Lr, k);
    for (int i = lo + (int)threadIdx.x; i <= hi; i += (int)blockDim.x) {
      const int j = k - i;
      int v;
      if (i == 0) v = j;
      else if (j == 0) v = i;
      else {
        const int sub = diag[a + i - 1] + (r[i - 1] != h[j - 1] ? 1 : 0);
        v = min(sub, min(diag[b + i - 1], diag[b + i]) + 1);
      }
      diag[c + i] = v;
    }
    __syncthreads();
    const int t = a; a = b; b = c; c = t;
  }
  return diag[b + Lr];
}

}  // namespace tavsr
