// The time stretch of DESIGN section 15, step 3, as sa_pitch_stretch_mag (sa_pitch.hip) and sa_pv_synth
// (sa_phasevoc.hip) both evaluate it: one text, so that the two write the same bits.
#pragma once
#include "sa_common.h"

#define PN_MAX_B 65535                   // grid.y
#define PN_MAX_T (1 << 23)               // the vocoder's bound
#define PN_NBIN 201

__device__ static inline float pn_ratio(float r) {         // a ratio no kernel can be led out of bounds by
  return r >= 0.5f && r <= 2.0f ? r : (r > 2.0f ? 2.0f : (r < 0.5f ? 0.5f : 1.0f));
}

// T'_b = ceil((T - 1) r_b) + 1 output frames carry signal
__device__ static inline int pn_frames(int T, double r) { return (int)ceil((double)(T - 1) * r) + 1; }

// output frame tp reads the position min(tp / r, T - 1) (fp64) between the frames i and i + 1, i <= T - 2: -> i,
// and the weight a of frame i + 1
__device__ static inline int pn_position(int tp, double r, int T, float* a) {
  const double pos = fmin((double)tp / r, (double)(T - 1));
  const int i = min((int)floor(pos), T - 2);
  *a = (float)(pos - (double)i);
  return i;
}

__device__ static inline float pn_mag(float2 p) { return sqrtf(fmaf(p.x, p.x, p.y * p.y)); }

__device__ static inline float pn_mix(float a, float mp, float mq) { return fmaf(a, mq, (1.0f - a) * mp); }
