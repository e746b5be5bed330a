// Pitch normalisation (pitchnorm.py): an F0 tracker and the three passes that, around the
// vocoder's Griffin-Lim, scale a waveform's pitch by a per-utterance ratio.  16 kHz, hop 160.  Four kernels:
//   sa_yin_f0             f0 [B][T] in Hz, T = N / 160 + 1: YIN (de Cheveigne & Kawahara 2002) in its direct form
//   sa_pitch_ratio        r_b = clamp(target / mean voiced f0), fp64, fixed order
//   sa_pitch_stretch_mag  |STFT| resampled along time to ceil((T - 1) r_b) + 1 frames (duration times r_b)
//   sa_pitch_resample     windowed-sinc read of the re-synthesised waveform at n r_b (duration back, pitch times r_b)
// Plain fp32 FMAs (positions and filter weights in fp64), no atomics, the same bits on every run.
#include "sa_common.h"
#include "sa_pitch_shared.h"
#include <errno.h>
#include <limits.h>

#define YIN_W 400                        // terms of a difference sum
#define YIN_L (YIN_W + PN_TMAX)          // samples a frame reads; frame t starts at 160 t - L / 2
#define YIN_G 8                          // frames per workgroup, one wave each
#define YIN_K 5                          // consecutive lags per lane (odd: the lanes' LDS reads hit 64 banks)
#define YIN_THREADS (YIN_G * SA_WAVE)
#define YIN_LAGS (YIN_K * SA_WAVE)       // 320 lag slots, 1..266 of them used
#define YIN_XS ((YIN_G - 1) * PN_HOP + YIN_W + YIN_LAGS + YIN_K + 3)   // 1848: what the idle slots read too
#define YIN_DP (YIN_LAGS + 2)            // d' slots per frame in LDS

extern "C" int sa_yin_dim(int which) {
  switch (which) {
    case 0: return PN_SR;
    case 1: return PN_HOP;
    case 2: return YIN_W;
    case 3: return PN_TMIN;
    case 4: return PN_TMAX;
    case 5: return YIN_L;
    case 6: return YIN_G;
    case 7: return RS_TILE;
    default: return -EINVAL;
  }
}

// ---- F0 ----------------------------------------------------------------------------------------------
// grid (tiles of 8 frames, B), 8 waves.  The workgroup stages the samples its 8 frames read (zeros outside
// [0, N)) once; wave f takes frame t0 + f, lane l the lags 5 l + 1 .. 5 l + 5.  Per j the lane reads x[j] (one
// address per wave: a broadcast) and one new x[j + lag] into a sliding window of 9 registers, and makes five
// subtract-square-adds.  Then, per wave: the lanes' running sums and a shuffle scan give c(tau) in a fixed
// order; d' goes to LDS; every lane tests its five lags for the first dip and a butterfly takes the smallest;
// lane 0 interpolates in fp64 and rounds once.  Lag slots past 266 compute on staged (or zero) samples and are
// discarded.
__global__ __launch_bounds__(YIN_THREADS) void sa_yin_f0_kernel(const float* __restrict__ wav, int N, int T,
                                                                float thr, float* __restrict__ f0,
                                                                float* __restrict__ dprime) {
  __shared__ float xs[YIN_XS];
  __shared__ float dp[YIN_G][YIN_DP];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * YIN_G;
  const int f = tid >> 6, lane = tid & 63, t = t0 + f;
  const long long s0 = (long long)t0 * PN_HOP - YIN_L / 2;
  for (int i = tid; i < YIN_XS; i += YIN_THREADS) {
    const long long n = s0 + i;
    xs[i] = (n >= 0 && n < N) ? wav[(size_t)b * N + n] : 0.0f;
  }
  __syncthreads();

  const int tau0 = YIN_K * lane + 1;
  const float* x = xs + f * PN_HOP;
  float d[YIN_K], w[2 * YIN_K - 1];
#pragma unroll
  for (int k = 0; k < YIN_K; ++k) d[k] = 0.0f;
#pragma unroll
  for (int k = 0; k < YIN_K - 1; ++k) w[k] = x[tau0 + k];
#pragma unroll 2
  for (int j = 0; j < YIN_W; j += YIN_K) {
#pragma unroll
    for (int k = 0; k < YIN_K; ++k) w[YIN_K - 1 + k] = x[j + tau0 + YIN_K - 1 + k];
#pragma unroll
    for (int u = 0; u < YIN_K; ++u) {
      const float xj = x[j + u];
#pragma unroll
      for (int k = 0; k < YIN_K; ++k) {
        const float df = xj - w[u + k];
        d[k] = fmaf(df, df, d[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < YIN_K - 1; ++k) w[k] = w[YIN_K + k];
  }

  // c(tau): the lane's running sums, then an inclusive scan of the lanes' totals
  float run[YIN_K];
  run[0] = d[0];
#pragma unroll
  for (int k = 1; k < YIN_K; ++k) run[k] = run[k - 1] + d[k];
  float incl = run[YIN_K - 1];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  const float prev = __shfl_up(incl, 1, 64);
  const float base = lane == 0 ? 0.0f : prev;
  if (lane == 0) dp[f][0] = 1.0f;
#pragma unroll
  for (int k = 0; k < YIN_K; ++k) {
    const float c = base + run[k];
    dp[f][tau0 + k] = c > 0.0f ? d[k] * (float)(tau0 + k) / c : 1.0f;
  }
  if (lane == 0) dp[f][YIN_LAGS + 1] = 1.0f;
  __syncthreads();

  int pick = INT_MAX;
#pragma unroll
  for (int k = YIN_K - 1; k >= 0; --k) {
    const int tau = tau0 + k;
    const float c = dp[f][tau];
    if (tau >= PN_TMIN && tau < PN_TMAX && c < thr && c <= dp[f][tau - 1] && c < dp[f][tau + 1]) pick = tau;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pick = min(pick, __shfl_xor(pick, o, 64));

  if (t >= T) return;
  if (dprime) {
    float* out = dprime + ((size_t)b * T + t) * (PN_TMAX + 1);
    for (int i = lane; i <= PN_TMAX; i += 64) out[i] = dp[f][i];
  }
  if (lane == 0) {
    float hz = 0.0f;
    if (pick != INT_MAX) hz = pn_refined_hz(pick, dp[f][pick - 1], dp[f][pick], dp[f][pick + 1]);
    f0[(size_t)b * T + t] = hz;
  }
}

extern "C" int sa_yin_f0(const float* wav, int B, int N, float threshold, float* f0, float* dprime, void* stream) {
  if (!wav || !f0 || !pn_rows_ok(B) || !pn_samples_ok(N)) return -EINVAL;
  const int T = N / PN_HOP + 1;
  hipLaunchKernelGGL(sa_yin_f0_kernel, dim3(sa_div_up(T, YIN_G), B), dim3(YIN_THREADS), 0, (hipStream_t)stream, wav,
                     N, T, threshold, f0, dprime);
  return -(int)hipGetLastError();
}

// ---- ratio -------------------------------------------------------------------------------------------
// grid (B): one workgroup per row.  The first F_b = round(lens_b N) / 160 + 1 frames count; their voiced mean is
// pn_voiced_mean's (sa_pitch_shared.h: sa_pitch_contour writes the same bits).
__global__ __launch_bounds__(256) void sa_pitch_ratio_kernel(const float* __restrict__ f0,
                                                             const float* __restrict__ lens, int T, int N,
                                                             double target, double r_min, double r_max,
                                                             int min_voiced, float* __restrict__ ratio,
                                                             float* __restrict__ mean, int* __restrict__ voiced) {
  const int b = blockIdx.x;
  int v;
  const double m = pn_voiced_mean(f0 + (size_t)b * T, pn_counted_frames(lens[b], N, T), &v);
  if (threadIdx.x == 0) {
    double r = 1.0;
    if (v >= min_voiced && m > 0.0) r = fmin(fmax(target / m, r_min), r_max);
    ratio[b] = (float)r;
    mean[b] = (float)m;
    voiced[b] = v;
  }
}

extern "C" int sa_pitch_ratio(const float* f0, const float* lens, int B, int T, int N, float target, float r_min,
                              float r_max, int min_voiced, float* ratio, float* mean, int* voiced, void* stream) {
  if (!f0 || !lens || !ratio || !mean || !voiced || !pn_rows_ok(B) || !pn_frames_ok(T, 1) || !pn_samples_ok(N) ||
      !(target > 0.0f) || !(r_min >= 0.5f) || !(r_max <= 2.0f) || !(r_min <= r_max))
    return -EINVAL;
  hipLaunchKernelGGL(sa_pitch_ratio_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, f0, lens, T, N,
                     (double)target, (double)r_min, (double)r_max, min_voiced, ratio, mean, voiced);
  return -(int)hipGetLastError();
}

// ---- stretch -----------------------------------------------------------------------------------------
// grid (chunks of 256 elements of a row's [Tout][201], B).  Output frame t' < T'_b = ceil((T - 1) r_b) + 1 reads
// the position min(t' / r_b, T - 1) (fp64) between the frames i and i + 1; the frames from T'_b on are zero.
__global__ __launch_bounds__(256) void sa_pitch_stretch_mag_kernel(const float2* __restrict__ R,
                                                                   const float* __restrict__ ratio, int T, int Tout,
                                                                   float* __restrict__ S) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= Tout * PN_NBIN) return;
  const int tp = e / PN_NBIN, k = e - tp * PN_NBIN;
  const double r = (double)pn_ratio(ratio[b]);
  float v = 0.0f;
  if (tp < pn_frames(T, r)) {
    float a;
    const int i = pn_position(tp, r, T, &a);
    const float2 p = R[((size_t)b * T + i) * PN_NBIN + k], q = R[((size_t)b * T + i + 1) * PN_NBIN + k];
    v = pn_mix(a, pn_mag(p), pn_mag(q));           // (sa_pitch_stretch.h: sa_pv_synth writes the same bits)
  }
  S[((size_t)b * Tout) * PN_NBIN + e] = v;
}

extern "C" int sa_pitch_stretch_mag(const void* R, const float* ratio, int B, int T, int Tout, float* S,
                                    void* stream) {
  if (!R || !ratio || !S || !pn_rows_ok(B) || !pn_frames_ok(T, 2) || !pn_frames_ok(Tout, 1)) return -EINVAL;
  hipLaunchKernelGGL(sa_pitch_stretch_mag_kernel, dim3(sa_div_up(Tout * PN_NBIN, 256), B), dim3(256), 0,
                     (hipStream_t)stream, (const float2*)R, ratio, T, Tout, S);
  return -(int)hipGetLastError();
}

// ---- resample ----------------------------------------------------------------------------------------
// grid (tiles of 256 outputs, B).  out[n] = sum_i y[i] h(n r - i), h(u) = c sinc(c u) (0.5 + 0.5 cos(pi u / H)) on
// |u| < H, c = min(1, 1 / r), H = 16 / c: at most 64 taps.  Row b's input ends at 160 ceil(ceil(Nout / 160) r_b)
// samples (the stretched frame count of a waveform of Nout samples), at most Nin.  The workgroup stages the
// input span of its tile (at most 2 256 + 64 + 2 samples, zeros outside the row's input); a thread forms each
// weight in fp64 and rounds it once, and accumulates in fp32 in the order of i (pn_rs_taps, sa_pitch_shared.h:
// sa_pitch_resample_map runs the same loop).
__global__ __launch_bounds__(RS_TILE) void sa_pitch_resample_kernel(const float* __restrict__ y,
                                                                    const float* __restrict__ ratio,
                                                                    const int* __restrict__ n_valid, int Nin,
                                                                    int Nout, float* __restrict__ out) {
  __shared__ float ys[RS_SPAN];
  const int tid = threadIdx.x, b = blockIdx.y, n0 = blockIdx.x * RS_TILE, n = n0 + tid;
  const double r = (double)pn_ratio(ratio[b]);
  double H;
  pn_rs_cutoff(r, &H);
  const long long vin = min((long long)Nin, 160LL * (long long)ceil((double)((Nout + PN_HOP - 1) / PN_HOP) * r));
  const long long span0 = (long long)floor((double)n0 * r - H) + 1;
  for (int i = tid; i < RS_SPAN; i += RS_TILE) {
    const long long s = span0 + i;
    ys[i] = (s >= 0 && s < vin) ? y[(size_t)b * Nin + s] : 0.0f;
  }
  __syncthreads();
  if (n >= Nout) return;
  out[(size_t)b * Nout + n] = n < n_valid[b] ? pn_rs_taps<false>(ys, span0, (double)n * r, r) : 0.0f;
}

extern "C" int sa_pitch_resample(const float* y, const float* ratio, const int* n_valid, int B, int Nin, int Nout,
                                 float* out, void* stream) {
  if (!y || !ratio || !n_valid || !out || !pn_rows_ok(B) || !pn_samples_ok(Nin) || Nout < 1 || Nout > PN_MAX_N / 2)
    return -EINVAL;
  hipLaunchKernelGGL(sa_pitch_resample_kernel, dim3(sa_div_up(Nout, RS_TILE), B), dim3(RS_TILE), 0,
                     (hipStream_t)stream, y, ratio, n_valid, Nin, Nout, out);
  return -(int)hipGetLastError();
}
