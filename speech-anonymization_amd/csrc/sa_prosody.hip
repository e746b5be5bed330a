// Pitch-correlation scoring (ops.f0_compare): f0_ref, f0_deg [B][T] fp32 in Hz (0 or less:
// unvoiced), frames [B] -> rho, shift_st, dev_st, voicing [B] fp32, lag, common [B] int32.  Every step in fp64
// (include/sa_hip.h carries the definition):
//   per lag   l in [-Lg, Lg]: over the frames voiced in both tracks, ref at t against deg at t + l, the means in one
//             pass and the centred sums s_xx, s_yy, s_xy in a second; rho_l = s_xy / sqrt(s_xx s_yy)
//   choice    the lags walked as 0, -1, +1, ..., -Lg, +Lg: the first valid one whose rho is above every earlier one
//   at l*     e = 12 log2(y / x): its mean and standard deviation, and the share of frames whose voicing agrees
// One workgroup of 16 waves per row.  Wave w takes the lags at the positions w, w + 16, ... of the walk; lane i the
// frames lo + i, lo + i + 64, ... of the overlap in order, the wave by butterfly.  The per-lag results go to LDS; after
// the one barrier wave 0 walks them and evaluates l*.  The tracks are read from memory at every lag: at T = 1001 a row's
// two tracks are 8 KB, inside the 32 KB of a CU's vector L1, and a staged copy would need a second path above
// T = 16000.  No atomics, every sum in a fixed order: the same bits on every run.
#include "sa_pitch_shared.h"
#include <errno.h>

#define PR_MAX_LAG 32
#define PR_LAGS (2 * PR_MAX_LAG + 1)
#define PR_THREADS 1024
#define PR_WAVES (PR_THREADS / 64)
#define PR_MAX_T 104858                   // the frames of 2^24 samples

extern "C" int sa_f0cmp_dim(int which) {
  switch (which) {
    case 0: return PN_HOP;
    case 1: return PR_MAX_LAG;
    case 2: return PR_THREADS;
    default: return -EINVAL;
  }
}

__device__ static inline int pr_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// position p of the walk 0, -1, +1, -2, +2, ... -> the lag
__device__ static inline int pr_lag(int p) { return (p & 1) ? -((p + 1) >> 1) : (p >> 1); }

// the shift of a frame in semitones, rounded once as a product (no contraction into the subtraction that follows)
__device__ static inline double pr_semitones(float a, float c) { return __dmul_rn(12.0, log2((double)c / (double)a)); }

// grid B
__global__ __launch_bounds__(PR_THREADS) void sa_f0_compare_kernel(const float* __restrict__ f0_ref,
                                                                    const float* __restrict__ f0_deg,
                                                                    const int* __restrict__ frames, int T, int Lg,
                                                                    int min_common, float* __restrict__ rho,
                                                                    int* __restrict__ lag, int* __restrict__ common,
                                                                    float* __restrict__ shift_st,
                                                                    float* __restrict__ dev_st,
                                                                    float* __restrict__ voicing) {
  __shared__ double s_rho[PR_LAGS];
  __shared__ int s_n[PR_LAGS];                              // the pairs of a valid lag, 0 for one that is not
  __shared__ int s_agree[PR_LAGS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.x;
  const int F = min(max(frames[b], 0), T);
  const float* x = f0_ref + (size_t)b * T;
  const float* y = f0_deg + (size_t)b * T;
  for (int p = wv; p < 2 * Lg + 1; p += PR_WAVES) {         // (uniform per wave)
    const int l = pr_lag(p);
    const int lo = max(0, -l), hi = min(F, F - l);          // 0 <= t < F and 0 <= t + l < F
    double sx = 0.0, sy = 0.0;
    int n = 0, agree = 0;
    for (int t = lo + lane; t < hi; t += 64) {
      const float a = x[t], c = y[t + l];
      const bool va = a > 0.0f, vc = c > 0.0f;
      agree += va == vc;
      if (va && vc) {
        sx += (double)a;
        sy += (double)c;
        ++n;
      }
    }
    sx = sa_wave_sum_d(sx), sy = sa_wave_sum_d(sy);
    n = pr_wave_sum_i(n), agree = pr_wave_sum_i(agree);
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    if (n >= min_common) {
      const double mx = sx / (double)n, my = sy / (double)n;
      for (int t = lo + lane; t < hi; t += 64) {
        const float a = x[t], c = y[t + l];
        if (a > 0.0f && c > 0.0f) {
          const double dx = (double)a - mx, dy = (double)c - my;
          sxx = fma(dx, dx, sxx);
          syy = fma(dy, dy, syy);
          sxy = fma(dx, dy, sxy);
        }
      }
      sxx = sa_wave_sum_d(sxx), syy = sa_wave_sum_d(syy), sxy = sa_wave_sum_d(sxy);
    }
    if (lane == 0) {
      const bool valid = n >= min_common && sxx > 0.0 && syy > 0.0;
      s_rho[p] = valid ? sxy / sqrt(sxx * syy) : 0.0;
      s_n[p] = valid ? n : 0;
      s_agree[p] = agree;
    }
  }
  __syncthreads();
  if (wv != 0) return;
  int best = -1;
  double r = 0.0;
  for (int p = 0; p < 2 * Lg + 1; ++p)
    if (s_n[p] > 0 && (best < 0 || s_rho[p] > r)) best = p, r = s_rho[p];
  int l = 0, n = 0;
  double shift = 0.0, dev = 0.0;
  double share = F > 0 ? (double)s_agree[0] / (double)F : 0.0;
  if (best >= 0) {
    l = pr_lag(best), n = s_n[best];
    const int lo = max(0, -l), hi = min(F, F - l);
    double se = 0.0;
    for (int t = lo + lane; t < hi; t += 64) {
      const float a = x[t], c = y[t + l];
      if (a > 0.0f && c > 0.0f) se += pr_semitones(a, c);
    }
    shift = sa_wave_sum_d(se) / (double)n;
    double sd = 0.0;
    for (int t = lo + lane; t < hi; t += 64) {
      const float a = x[t], c = y[t + l];
      if (a > 0.0f && c > 0.0f) {
        const double d = pr_semitones(a, c) - shift;
        sd = fma(d, d, sd);
      }
    }
    dev = sqrt(sa_wave_sum_d(sd) / (double)n);
    share = (double)s_agree[best] / (double)(hi - lo);
  }
  if (lane == 0) {
    rho[b] = (float)r;
    if (lag) lag[b] = l;
    if (common) common[b] = n;
    if (shift_st) shift_st[b] = (float)shift;
    if (dev_st) dev_st[b] = (float)dev;
    if (voicing) voicing[b] = (float)share;
  }
}

extern "C" int sa_f0_compare(const float* f0_ref, const float* f0_deg, const int* frames, int B, int T, int max_lag,
                             int min_common, float* rho, int* lag, int* common, float* shift_st, float* dev_st,
                             float* voicing, void* stream) {
  if (!f0_ref || !f0_deg || !frames || !rho || !pn_rows_ok(B) || T < 1 || T > PR_MAX_T || max_lag < 0 ||
      max_lag > PR_MAX_LAG || min_common < 2)
    return -EINVAL;
  hipLaunchKernelGGL(sa_f0_compare_kernel, dim3(B), dim3(PR_THREADS), 0, (hipStream_t)stream, f0_ref, f0_deg, frames,
                     T, max_lag, min_common, rho, lag, common, shift_st, dev_st, voicing);
  return -(int)hipGetLastError();
}
