// LPC formant normalisation (formantnorm.py; ops.pole_warp, ops.formant_centre; DESIGN section 26;
// include/sa_hip.h carries the definition).
// sa_pole_warp: sa_mcadams's framing, fit, roots, filters, overlap-add and level matching, with
// one difference: the angle phi of a kept pole goes to
//   phi' = q phi                                                 for phi <= phi0
//   phi' = q phi0 + (pi - q phi0) (phi - phi0) / (pi - phi0)     above it,   phi0 = 0.85 pi min(1, 1 / q)
// a vocal-tract-length warp of the poles themselves: continuous, strictly increasing, (0, pi) onto itself; every
// resonance up to phi0 is scaled by q exactly.  |z| and the real poles are kept.
// sa_formant_centre: the lower medians of a row's three formant tracks over the frames scored and voiced, and the
// ratio q that brings their geometric mean to a target's; the medians by the bitwise radix select of
// sa_formant_compare_kernel on three keys.
// The frame and level kernels and the select's helpers are sa_lpc_shared.h's; this file holds the angle map and the
// centre kernel.  No atomics, every sum in a fixed order: the same bits on every run.
#include "sa_lpc_shared.h"

#define PW_KNEE_PERMILLE 850
#define PW_PI 3.14159265358979323846
#define FN_NF 3
#define FN_MAX_T 104858                  // the frames of 2^24 samples (sa_formant_dim(6))
#define FN_THREADS 1024
#define FN_WAVES (FN_THREADS / 64)
#define FN_FMIN 90.0f
#define FN_FMAX 5500.0f

extern "C" int sa_pole_warp_dim(int which) {
  switch (which) {
    case 0: return SA_FR_W;
    case 1: return SA_FR_H;
    case 2: return SA_FR_P;
    case 3: return SA_FR_G;
    case 4: return SA_FR_THREADS;
    case 5: return SA_LPC_ITERS;
    case 6: return SA_FR_CHUNK;
    case 7: return PW_KNEE_PERMILLE;
    default: return -EINVAL;
  }
}

struct SaPoleWarpMap {
  static constexpr bool COPIES = true;                      // q = 1: the row is copied and no frame is read
  __device__ static inline double clamp(float q) {          // a ratio no kernel can be led astray by
    return q >= 0.5f && q <= 2.0f ? (double)q : (q > 2.0f ? 2.0 : (q < 0.5f ? 0.5 : 1.0));
  }
  __device__ static inline double angle(double phi, double q) {
    const double phi0 = (0.001 * PW_KNEE_PERMILLE * PW_PI) * fmin(1.0, 1.0 / q), low = q * phi0;
    return phi <= phi0 ? q * phi : low + (PW_PI - low) * ((phi - phi0) / (PW_PI - phi0));
  }
};

extern "C" int sa_pole_warp(const float* wav, const float* q, const int* n_valid, int B, int N, int level, float* out,
                            void* ws, int* status, float* gain, void* stream) {
  return sa_fr_roots<SaPoleWarpMap>(wav, q, n_valid, B, N, level, out, ws, status, gain, stream);
}

// ---- the centre of a row's formants and the ratio to a target ---------------------------------------------
// grid B, one workgroup of 16 waves per row; thread i takes the frames i, i + 1024, ...  A first pass counts the
// frames that count; then 32 passes, one per bit of the key from the top, settle that bit of the three medians at
// once (sa_formant_compare_kernel's select).  f0 may be NULL: every frame voiced.
__global__ __launch_bounds__(FN_THREADS) void sa_formant_centre_kernel(
    const float* __restrict__ freq, const int* __restrict__ status, const float* __restrict__ f0,
    const int* __restrict__ frames, int T, float t1, float t2, float t3, float q_min, float q_max, int min_frames,
    float* __restrict__ med, float* __restrict__ q, int* __restrict__ count) {
  __shared__ int cnt[2][FN_WAVES][FN_NF];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int F = min(max(frames[b], 0), T);
  const size_t base = (size_t)b * T;
  const float* Fr = freq + base * FN_NF;
  const int* st = status + base;
  const float* pf = f0 ? f0 + base : nullptr;

  int c[FN_NF];
#pragma unroll
  for (int s = 0; s < FN_NF; ++s) c[s] = 0;
  for (int t = tid; t < F; t += FN_THREADS) c[0] += st[t] == 0 && (!pf || pf[t] > 0.0f);
  sa_sel_block_sum(c, cnt, 0);
  const int n = c[0];
  const bool scored = n >= min_frames;                      // (uniform)

  unsigned prefix[FN_NF];
  int want[FN_NF];
#pragma unroll
  for (int s = 0; s < FN_NF; ++s) prefix[s] = 0u, want[s] = (n - 1) / 2;
  if (scored) {
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned one = 1u << bit, mask = ~(one - 1u);   // the bits settled so far, and this one
#pragma unroll
      for (int s = 0; s < FN_NF; ++s) c[s] = 0;
      for (int t = tid; t < F; t += FN_THREADS) {
        if (st[t] == 0 && (!pf || pf[t] > 0.0f)) {
#pragma unroll
          for (int k = 0; k < FN_NF; ++k) c[k] += (sa_sel_key(Fr[(size_t)t * FN_NF + k]) & mask) == prefix[k];
        }
      }
      sa_sel_block_sum(c, cnt, bit & 1);                        // (31 -> 1 after the count's 0, then alternating)
#pragma unroll
      for (int s = 0; s < FN_NF; ++s)
        if (want[s] >= c[s]) want[s] -= c[s], prefix[s] |= one;
    }
  }
  if (tid != 0) return;
  const float tg[FN_NF] = {t1, t2, t3};
  double lg = 0.0;
#pragma unroll
  for (int k = 0; k < FN_NF; ++k) {
    const float m = scored ? sa_sel_value(prefix[k]) : 0.0f;
    if (med) med[(size_t)b * FN_NF + k] = m;
    lg += log((double)tg[k] / (double)m);
  }
  double v = exp(lg / 3.0);
  v = !(v == v) ? 1.0 : fmin(fmax(v, (double)q_min), (double)q_max);   // (a NaN: a median of 0 or less; no change)
  q[b] = scored ? (float)v : 1.0f;
  if (count) count[b] = scored ? n : 0;
}

extern "C" int sa_formant_centre(const float* freq, const int* status, const float* f0, const int* frames, int B, int T,
                                 float t1, float t2, float t3, float q_min, float q_max, int min_frames, float* med,
                                 float* q, int* count, void* stream) {
  if (!freq || !status || !frames || !q || B < 1 || B > SA_FR_MAX_B || T < 1 || T > FN_MAX_T || min_frames < 1)
    return -EINVAL;
  if (!(t1 >= FN_FMIN && t1 < t2 && t2 < t3 && t3 <= FN_FMAX)) return -EINVAL;
  if (!(q_min >= 0.5f && q_min <= 1.0f && q_max >= 1.0f && q_max <= 2.0f)) return -EINVAL;
  hipLaunchKernelGGL(sa_formant_centre_kernel, dim3(B), dim3(FN_THREADS), 0, (hipStream_t)stream, freq, status, f0,
                     frames, T, t1, t2, t3, q_min, q_max, min_frames, med, q, count);
  return -(int)hipGetLastError();
}
