// The time map of DESIGN section 20, steps 5 and 6, as sa_pitch_contour (sa_contour.hip) writes it and
// sa_pv_synth_map (sa_phasevoc.hip) and sa_pitch_resample_map (sa_contour.hip) read it: one text.  rho_q [B][T] int32
// is the per-frame ratio in units of 2^-16, Q [B][T] int64 the running sum of w[t] = rho_q[t] + rho_q[t + 1] (the
// mean ratio of hop interval t in units of 2^-17), Q[0] = 0.  The tables live on the device: every value read from
// them is clamped where it is read, and every index derived from them is clamped to its array.
#pragma once
#include "sa_common.h"

#define CT_RHO_ONE (1 << 16)             // ratio 1 in rho_q
#define CT_QBITS 17                      // one input frame in Q
#define CT_QONE (1LL << CT_QBITS)

__device__ static inline int ct_rho(int v) { return min(max(v, 1 << 15), 1 << 17); }

// w[t], t <= T - 2, in [2^16, 2^18].  (No __restrict__ on rq: sa_pitch_contour reads here, after a barrier, the
// rho_q its own workgroup has just written.)
__device__ static inline long long ct_w(const int* rq, int t) {
  const long long w = (long long)ct_rho(rq[t]) + (long long)ct_rho(rq[t + 1]);
  return min(max(w, 1LL << 16), 1LL << 18);
}

// Q[T - 1], in [0, (T - 1) 2^18]
__device__ static inline long long ct_end(const long long* __restrict__ Q, int T) {
  return min(max(Q[T - 1], 0LL), (long long)(T - 1) << 18);
}

// T'_b = ceil(Q[T - 1] / 2^17) + 1 output frames carry signal
__device__ static inline int ct_frames(const long long* __restrict__ Q, int T) {
  return (int)((ct_end(Q, T) + CT_QONE - 1) >> CT_QBITS) + 1;
}

// the largest i <= T - 2 with Q[i] <= X (0 when there is none)
__device__ static inline int ct_search(const long long* __restrict__ Q, int T, long long X) {
  int lo = 0, hi = T - 2;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (Q[mid] <= X) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// output frame tp reads between the frames i and i + 1, i <= T - 2: -> i, walked forward from the caller's i of an
// earlier frame (i never decreases), and the weight a of frame i + 1, in [0, 1]
__device__ static inline int ct_position(const long long* __restrict__ Q, const int* __restrict__ rq, int T, int tp,
                                         int i, float* a) {
  const long long X = (long long)tp << CT_QBITS;
  if (X >= ct_end(Q, T)) {
    *a = 1.0f;
    return T - 2;
  }
  i = min(max(i, 0), T - 2);
  while (i < T - 2 && Q[i + 1] <= X) ++i;
  const float v = (float)((double)(X - Q[i]) / (double)ct_w(rq, i));
  *a = v >= 0.0f ? fminf(v, 1.0f) : 0.0f;                    // (NaN -> 0)
  return i;
}
