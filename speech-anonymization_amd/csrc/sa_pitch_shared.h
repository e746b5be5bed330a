// The steps that more than one kernel of the pitch paths evaluates (DESIGN sections 15, 19, 20 and 21), each as one
// text, so that the kernels that share a step write the same bits:
//   the sample rate, hop, lag range and size bounds    sa_pitch.hip, sa_contour.hip, sa_f0track.hip, sa_phasevoc.hip
//   the time stretch of section 15, step 3             sa_pitch_stretch_mag, sa_pv_synth
//   the frames that count and their voiced mean        sa_pitch_ratio, sa_pitch_contour, sa_f0_viterbi (the frames)
//   the parabolic lag refinement                       sa_yin_f0, sa_f0_viterbi
//   the windowed-sinc tap loop                         sa_pitch_resample, sa_pitch_resample_map
#pragma once
#include "sa_common.h"

#define PN_SR 16000
#define PN_HOP 160
#define PN_TMIN 40                       // 400 Hz
#define PN_TMAX 266                      // 60 Hz
#define PN_MAX_B 65535                   // grid.y
#define PN_MAX_T (1 << 23)               // the vocoder's bound
#define PN_MAX_N (1 << 30)
#define PN_NBIN 201
#define RS_TILE 256                      // outputs per workgroup of sa_pitch_resample and sa_pitch_resample_map
#define RS_HALF 16.0                     // filter half-width in periods of the cut-off
#define RS_SPAN (2 * RS_TILE + 2 * 32 + 2)

// what the extern "C" entry points accept: rows, frames (at least `least` of them) and samples
static inline bool pn_rows_ok(int B) { return B >= 1 && B <= PN_MAX_B; }
static inline bool pn_frames_ok(int T, int least) { return T >= least && T <= PN_MAX_T; }
static inline bool pn_samples_ok(int N) { return N >= 1 && N <= PN_MAX_N; }

__device__ static inline float pn_ratio(float r) {         // a ratio no kernel can be led out of bounds by
  return r >= 0.5f && r <= 2.0f ? r : (r > 2.0f ? 2.0f : (r < 0.5f ? 0.5f : 1.0f));
}

// ---- stretch -----------------------------------------------------------------------------------------
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

// ---- the frames that count ---------------------------------------------------------------------------
// The first F = round(len N) / 160 + 1 frames of a row count, at most T.
__device__ static inline int pn_counted_frames(float len, int N, int T) {
  double nb = rint((double)len * (double)N);
  nb = nb >= 0.0 ? (nb <= (double)N ? nb : (double)N) : 0.0;           // (NaN -> 0)
  const int F = (int)nb / PN_HOP + 1;
  return F > T ? T : F;
}

// The mean of the voiced frames (f0 > 0) among the first F of a row, by a workgroup of 256 threads: every thread adds
// its strided frames in fp64, the wave adds its lanes by butterfly, thread 0 adds the 4 waves in order.  -> in thread 0
// the mean (0 when no frame is voiced) and in *voiced the count; the other threads get zeros.  Holds a barrier: every
// thread of the workgroup calls it.
__device__ static inline double pn_voiced_mean(const float* __restrict__ f0, int F, int* voiced) {
  __shared__ double part[4];
  __shared__ int cnt[4];
  const int tid = threadIdx.x;
  double acc = 0.0;
  int n = 0;
  for (int t = tid; t < F; t += 256) {
    const float v = f0[t];
    if (v > 0.0f) {
      acc += (double)v;
      ++n;
    }
  }
  acc = sa_wave_sum_d(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((tid & 63) == 0) {
    part[tid >> 6] = acc;
    cnt[tid >> 6] = n;
  }
  __syncthreads();
  double m = 0.0;
  int v = 0;
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < 4; ++w) {
      s += part[w];
      v += cnt[w];
    }
    if (v > 0) m = s / (double)v;
  }
  *voiced = v;
  return m;
}

// ---- lag refinement ----------------------------------------------------------------------------------
// The lag tau of a dip of d' moved to the vertex of the parabola through d'[tau - 1], d'[tau], d'[tau + 1] (fp64; no
// move where the three do not curve upwards), as a frequency rounded once.
__device__ static inline float pn_refined_hz(int tau, float below, float at, float above) {
  const double a = below, c = at, e = above;
  const double den = a - 2.0 * c + e;
  const double off = den > 0.0 ? 0.5 * (a - e) / den : 0.0;
  return (float)((double)PN_SR / ((double)tau + off));
}

// ---- resampler ---------------------------------------------------------------------------------------
// h(u) = c sinc(c u) (0.5 + 0.5 cos(pi u / H)) on |u| < H at the ratio r: -> the cut-off c = min(1, 1 / r), and in *H
// the half-width 16 / c <= 32 in input samples
__device__ static inline double pn_rs_cutoff(double r, double* H) {
  const double c = r > 1.0 ? 1.0 / r : 1.0;
  *H = RS_HALF / c;
  return c;
}

// sum_i ys[i - span0] h(pos - i) over the at most 64 taps i > pos - H, for a read position pos at the ratio r; ys holds
// the RS_SPAN input samples from span0 on.  Each weight is formed in fp64 and rounded once, and the sum runs in fp32 in
// the order of i.  The first tap past the span ends the sum; a tap below the span is left out (SKIP_BELOW, what
// sa_pitch_resample_map needs for a table no sa_pitch_contour wrote) or ends the sum as well.
// Both callers get from this text the bits their own loops gave:
//   sa_pitch_resample ends the sum at a tap below the span.  There is none: the first tap is lo = floor(n r - H) + 1
//     and span0 = floor(n0 r - H) + 1 with n >= n0 and r > 0, so lo >= span0.  The two forms therefore give it the same
//     bits; it keeps the `break`, with which the kernel measured 2 % faster (0.620 ms against 0.633 ms at 32 x 10 s).
//   sa_pitch_resample_map had u = (double)(ip - i) + fr with pos = (double)ip + fr.  That pos is exact (|ip| < 2^31
//     and fr has 17 fraction bits: 48 bits), and so is pos - (double)i, whose value (ip - i) + fr has |ip - i| <= 64
//     and the same 17 fraction bits: both expressions give that value unrounded.
template <bool SKIP_BELOW>
__device__ static inline float pn_rs_taps(const float* ys, long long span0, double pos, double r) {
  double H;
  const double c = pn_rs_cutoff(r, &H);
  const long long lo = (long long)floor(pos - H) + 1;
  const double invH = 1.0 / H;
  // the first tap's place in ys as an int: in sa_pitch_resample 0 <= lo - span0 < RS_SPAN; from a table nobody checked
  // it can be anything, and is clamped to where all 64 taps lie below the span, or the first one past it
  const int first = SKIP_BELOW ? (int)min(max(lo - span0, -64LL), (long long)RS_SPAN) : (int)(lo - span0);
  float acc = 0.0f;
  for (int q = 0; q < 64; ++q) {
    const long long i = lo + q;
    const double u = pos - (double)i;
    const int idx = first + q;
    if (!(u > -H) || (!SKIP_BELOW && idx < 0) || idx >= RS_SPAN) break;
    if (SKIP_BELOW && idx < 0) continue;
    const double cu = c * u;
    const double snc = cu == 0.0 ? 1.0 : sinpi(cu) / (3.14159265358979323846 * cu);
    const float h = (float)(c * snc * (0.5 + 0.5 * cospi(u * invH)));
    acc = fmaf(ys[idx], h, acc);
  }
  return acc;
}
