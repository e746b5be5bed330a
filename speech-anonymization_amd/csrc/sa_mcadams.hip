// McAdams-coefficient anonymisation (mcadams.py): per frame of 320 samples at hop 160 under the
// periodic sqrt-Hann window, an order-20 LPC fit, every complex pole's angle phi raised to the power alpha, and the
// frame re-synthesised from its own residual; then overlap-add and RMS level matching.  Steps in fp64, the frame
// store and the output in fp32:
//   f = w x;  r_k = sum_j f[j] f[j + k];  r_0 < 1e-10: silent (status 1), rec = f;  r_0 *= 1 + 1e-9
//   a = Levinson-Durbin(r);  some |k_i| >= 1 or an error <= 0: fallback (status 2), rec = f
//   z = the 20 roots of a by Aberth-Ehrlich, one lane per root, at most 64 iterations, stop under 1e-14
//   a' = prod_{real}(1 - Re z x) prod_{Im z > 0}(1 - 2 |z| cos(phi^alpha) x + |z|^2 x^2);  a count that does not add
//        up to 20 or no convergence: fallback
//   res = FIR(a) f;  rec = IIR(1 / a') res;  F_t = fp32(rec w)
//   y[n] = F_t0[n - 160 t0 + 160] + F_{t0 + 1}[n - 160 t0], t0 = n / 160 (a gather);  out = fp32(g y)
// No atomics, every sum in a fixed order: the same bits on every run.
#include "sa_common.h"
#include <errno.h>

#define MC_W 320
#define MC_H 160
#define MC_P 20
#define MC_G 1                           // frames per workgroup: one wave each
#define MC_THREADS 64
#define MC_ITERS 64
#define MC_CHUNK 4096                    // samples per block of the level sums
#define MC_SUM_THREADS 256
#define MC_APPLY 1024                    // samples per block of the last pass
#define MC_MAX_B 65535                   // grid.y
#define MC_MAX_T (1 << 23)               // the vocoder's bound
#define MC_MAX_N (1 << 30)
#define MC_SILENCE 1e-10
#define MC_TOL2 1e-28                    // (1e-14)^2
#define MC_REAL 1e-6

extern "C" int sa_mcadams_dim(int which) {
  switch (which) {
    case 0: return MC_W;
    case 1: return MC_H;
    case 2: return MC_P;
    case 3: return MC_G;
    case 4: return MC_THREADS;
    case 5: return MC_ITERS;
    case 6: return MC_CHUNK;
    default: return -EINVAL;
  }
}

__device__ static inline double mc_alpha(float a) {         // a coefficient no kernel can be led astray by
  return a >= 0.25f && a <= 2.0f ? (double)a : (a > 2.0f ? 2.0 : (a < 0.25f ? 0.25 : 1.0));
}

__device__ static inline double mc_window(int j) { return sqrt(0.5 - 0.5 * cospi((double)j * (1.0 / 160.0))); }

// grid (T, B), one wave.  LDS: the windowed frame with 20 zeros on either side (the FIR's history and the
// autocorrelation's far end read zeros instead of branching), the residual, the output.  Lanes of a wave read
// consecutive doubles (one 256-byte bank row per 32 lanes: no conflict) or one address (a broadcast); the IIR keeps
// its 20-sample history in registers and reads the residual by broadcast.
//   (a) lane j mod 64 windows five samples
//   (b) lane (k, part) sums lag k over a third of the frame; the three parts are added in order
//   (c) every lane runs the Levinson recursion on the same values (the coefficients are then in registers for d, f)
//   (d) lane j < 20 owns root j: Horner for p and p', the Aberth sum over the other 19 by lane reads
//   (e) lane i owns coefficient i of a' while the 20 factors are multiplied in, one per step
//   (f) FIR: five outputs per lane;  IIR: the 320-step recursion, the same in every lane
__global__ __launch_bounds__(MC_THREADS) void sa_mcadams_frame_kernel(const float* __restrict__ wav,
                                                                       const float* __restrict__ alpha,
                                                                       const int* __restrict__ n_valid, int N, int T,
                                                                       float* __restrict__ ws,
                                                                       int* __restrict__ status) {
  __shared__ double fs[MC_P + MC_W + MC_P];
  __shared__ double rs[MC_W];
  __shared__ double ys[MC_W];
  __shared__ double part[MC_THREADS];
  __shared__ double a2s[MC_P + 1];
  const int lane = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
  const double al = mc_alpha(alpha[b]);
  if (al == 1.0) {                                          // the row is copied by the last pass; no frame is read
    if (status && lane == 0) status[(size_t)b * T + t] = 0;
    return;
  }
  const int nv = min(max(n_valid[b], 0), N);
  float* F = ws + ((size_t)b * T + t) * MC_W;

  // (a)
  double wv[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + 64 * i, n = MC_H * t - MC_H + j;
    const double x = n >= 0 && n < nv ? (double)wav[(size_t)b * N + n] : 0.0;
    wv[i] = mc_window(j);
    fs[MC_P + j] = wv[i] * x;
  }
  if (lane < MC_P) fs[lane] = 0.0, fs[MC_P + MC_W + lane] = 0.0;
  __syncthreads();

  // (b)
  {
    const int k = lane % (MC_P + 1), p = min(lane / (MC_P + 1), 2), j0 = 107 * p, j1 = min(MC_W, j0 + 107);
    double acc = 0.0;
    for (int j = j0; j < j1; ++j) acc = fma(fs[MC_P + j], fs[MC_P + j + k], acc);
    part[lane] = lane < 3 * (MC_P + 1) ? acc : 0.0;
  }
  __syncthreads();
  double r[MC_P + 1];
#pragma unroll
  for (int k = 0; k <= MC_P; ++k) r[k] = (part[k] + part[MC_P + 1 + k]) + part[2 * (MC_P + 1) + k];

  int st = r[0] < MC_SILENCE ? 1 : 0;
  double a[MC_P + 1];
  if (st == 0) {                                            // (uniform: every lane holds the same r)
    // (c)
    r[0] *= 1.0 + 1e-9;
    double err = r[0];
    bool bad = false;
    a[0] = 1.0;
#pragma unroll
    for (int i = 1; i <= MC_P; ++i) a[i] = 0.0;
#pragma unroll
    for (int m = 1; m <= MC_P; ++m) {
      double acc = r[m];
#pragma unroll
      for (int i = 1; i < m; ++i) acc = fma(a[i], r[m - i], acc);
      const double k = -acc / err;
      bad = bad || !(fabs(k) < 1.0);
      double prev[MC_P + 1];
#pragma unroll
      for (int i = 1; i < m; ++i) prev[i] = a[i];
#pragma unroll
      for (int i = 1; i < m; ++i) a[i] = fma(k, prev[m - i], prev[i]);
      a[m] = k;
      err *= 1.0 - k * k;
      bad = bad || !(err > 0.0);
    }
    if (bad) st = 2;
  }

  if (st == 0) {
    // (d)
    const bool mine = lane < MC_P;
    double zr, zi;
    {
      double s, c;
      sincospi(((double)lane + 0.25) * (2.0 / MC_P), &s, &c);
      zr = mine ? 0.9 * c : 2.0 + (double)lane;             // the idle lanes sit far away, apart from each other
      zi = mine ? 0.9 * s : 0.0;
    }
    bool conv = false;
    for (int it = 0; it < MC_ITERS && !conv; ++it) {
      double pr = 1.0, pi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
      for (int k = 1; k <= MC_P; ++k) {
        const double tr = fma(dr, zr, fma(-di, zi, pr)), ti = fma(dr, zi, fma(di, zr, pi));
        dr = tr, di = ti;
        const double ur = fma(pr, zr, fma(-pi, zi, a[k])), ui = fma(pr, zi, pi * zr);
        pr = ur, pi = ui;
      }
      const double dm = 1.0 / fma(dr, dr, di * di);
      const double qr = fma(pr, dr, pi * di) * dm, qi = fma(pi, dr, -pr * di) * dm;      // p / p'
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int k = 0; k < MC_P; ++k) {
        const double er = zr - __shfl(zr, k, 64), ei = zi - __shfl(zi, k, 64);
        const double m = 1.0 / fma(er, er, ei * ei);
        if (k != lane) sr = fma(er, m, sr), si = fma(-ei, m, si);
      }
      const double gr = 1.0 - fma(qr, sr, -qi * si), gi = -fma(qr, si, qi * sr);          // 1 - (p / p') sum
      const double gm = 1.0 / fma(gr, gr, gi * gi);
      const double cr = fma(qr, gr, qi * gi) * gm, ci = fma(qi, gr, -qr * gi) * gm;
      zr -= cr, zi -= ci;
      conv = !__any(mine && !(fma(cr, cr, ci * ci) < MC_TOL2));
    }
    const double m2 = fma(zr, zr, zi * zi), mod = sqrt(m2);
    const bool real = mine && fabs(zi) <= MC_REAL * mod, up = mine && zi > MC_REAL * mod;
    const int nreal = __popcll(__ballot(real)), nup = __popcll(__ballot(up));
    if (!conv || 2 * nup + nreal != MC_P) st = 2;

    if (st == 0) {
      // (e)
      double c1 = 0.0, c2 = 0.0;
      if (real) c1 = -zr;
      if (up) c1 = -2.0 * mod * cos(pow(atan2(zi, zr), al)), c2 = m2;
      double p = lane == 0 ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < MC_P; ++k) {
        const double k1 = __shfl(c1, k, 64), k2 = __shfl(c2, k, 64);
        const double u1 = __shfl_up(p, 1, 64), u2 = __shfl_up(p, 2, 64);
        p = fma(k2, lane >= 2 ? u2 : 0.0, fma(k1, lane >= 1 ? u1 : 0.0, p));
      }
      if (lane <= MC_P) a2s[lane] = p;

      // (f)
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int j = lane + 64 * i;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k <= MC_P; ++k) acc = fma(a[k], fs[MC_P + j - k], acc);
        rs[j] = acc;
      }
    }
  }
  __syncthreads();
  if (st == 0) {
    double c[MC_P + 1], h[MC_P];
#pragma unroll
    for (int k = 1; k <= MC_P; ++k) c[k] = a2s[k], h[k - 1] = 0.0;
    for (int jb = 0; jb < MC_W; jb += MC_P) {
#pragma unroll
      for (int u = 0; u < MC_P; ++u) {                      // h[(j - k) mod 20] is sample j - k
        double s = rs[jb + u];
#pragma unroll
        for (int k = 1; k <= MC_P; ++k) s = fma(-c[k], h[(u - k + MC_P) % MC_P], s);
        h[u] = s;
        ys[jb + u] = s;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + 64 * i;
    F[j] = (float)((st == 0 ? ys[j] : fs[MC_P + j]) * wv[i]);
  }
  if (status && lane == 0) status[(size_t)b * T + t] = st;
}

__device__ static inline float mc_y(const float* __restrict__ Fr, int n) {
  const int t0 = n / MC_H, o = n - MC_H * t0;
  return Fr[(size_t)t0 * MC_W + o + MC_H] + Fr[(size_t)(t0 + 1) * MC_W + o];
}

// grid (blocks of 4096 samples, B): sums[b][blk] = (sum x^2, sum y^2) over the block's samples below n_valid, each
// thread its 16 samples in order, the wave by butterfly, the four waves in order
__global__ __launch_bounds__(MC_SUM_THREADS) void sa_mcadams_sums_kernel(const float* __restrict__ wav,
                                                                          const float* __restrict__ alpha,
                                                                          const int* __restrict__ n_valid, int N,
                                                                          int T, const float* __restrict__ ws,
                                                                          double* __restrict__ sums) {
  __shared__ double sh[2 * (MC_SUM_THREADS / 64)];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (mc_alpha(alpha[b]) == 1.0) return;
  const int nv = min(max(n_valid[b], 0), N);
  const float* Fr = ws + (size_t)b * T * MC_W;
  double sx = 0.0, sy = 0.0;
  for (int i = 0; i < MC_CHUNK / MC_SUM_THREADS; ++i) {
    const int n = blockIdx.x * MC_CHUNK + i * MC_SUM_THREADS + tid;
    if (n < nv) {
      const double x = (double)wav[(size_t)b * N + n], y = (double)mc_y(Fr, n);
      sx = fma(x, x, sx), sy = fma(y, y, sy);
    }
  }
  sx = sa_wave_sum_d(sx), sy = sa_wave_sum_d(sy);
  if ((tid & 63) == 0) sh[2 * (tid >> 6)] = sx, sh[2 * (tid >> 6) + 1] = sy;
  __syncthreads();
  if (tid == 0) {
    double* o = sums + 2 * ((size_t)b * gridDim.x + blockIdx.x);
    o[0] = ((sh[0] + sh[2]) + sh[4]) + sh[6];
    o[1] = ((sh[1] + sh[3]) + sh[5]) + sh[7];
  }
}

// grid B, one wave: lane l adds the blocks l, l + 64, ... in order, the wave by butterfly;
// g = sqrt(sum x^2 / sum y^2), 1 when either is 0, when level is off, or when alpha is 1
__global__ __launch_bounds__(64) void sa_mcadams_gain_kernel(const float* __restrict__ alpha,
                                                             const double* __restrict__ sums, int nblk, int level,
                                                             double* __restrict__ g, float* __restrict__ gain) {
  const int lane = threadIdx.x, b = blockIdx.x;
  double v = 1.0;
  if (level && mc_alpha(alpha[b]) != 1.0) {                 // (uniform)
    double sx = 0.0, sy = 0.0;
    for (int i = lane; i < nblk; i += 64) {
      sx += sums[2 * ((size_t)b * nblk + i)];
      sy += sums[2 * ((size_t)b * nblk + i) + 1];
    }
    sx = sa_wave_sum_d(sx), sy = sa_wave_sum_d(sy);
    if (sx > 0.0 && sy > 0.0) v = sqrt(sx / sy);
  }
  if (lane == 0) {
    g[b] = v;
    if (gain) gain[b] = (float)v;
  }
}

// grid (blocks of 1024 samples, B): out = fp32(g y) below n_valid (the input itself when alpha is 1), 0 from there on
__global__ __launch_bounds__(256) void sa_mcadams_apply_kernel(const float* __restrict__ wav,
                                                               const float* __restrict__ alpha,
                                                               const int* __restrict__ n_valid, int N, int T,
                                                               const float* __restrict__ ws,
                                                               const double* __restrict__ g,
                                                               float* __restrict__ out) {
  const int b = blockIdx.y;
  const bool copy = mc_alpha(alpha[b]) == 1.0;
  const int nv = min(max(n_valid[b], 0), N);
  const float* Fr = ws + (size_t)b * T * MC_W;
  const double gb = g[b];
#pragma unroll
  for (int i = 0; i < MC_APPLY / 256; ++i) {
    const int n = blockIdx.x * MC_APPLY + i * 256 + threadIdx.x;
    if (n < N) {
      float v = 0.0f;
      if (n < nv) v = copy ? wav[(size_t)b * N + n] : (float)(gb * (double)mc_y(Fr, n));
      out[(size_t)b * N + n] = v;
    }
  }
}

extern "C" int sa_mcadams(const float* wav, const float* alpha, const int* n_valid, int B, int N, int level,
                          float* out, void* ws, int* status, float* gain, void* stream) {
  if (!wav || !alpha || !n_valid || !out || !ws || B < 1 || B > MC_MAX_B || N < 1 || N > MC_MAX_N) return -EINVAL;
  const int T = (N + MC_H - 1) / MC_H + 1;
  if (T > MC_MAX_T) return -EINVAL;
  const int nblk = sa_div_up(N, MC_CHUNK);
  float* F = (float*)ws;
  double* sums = (double*)(F + (size_t)B * T * MC_W);       // 1280 bytes per frame: 8-byte aligned
  double* g = sums + 2 * (size_t)B * nblk;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sa_mcadams_frame_kernel, dim3(T, B), dim3(MC_THREADS), 0, s, wav, alpha, n_valid, N, T, F,
                     status);
  if (level)
    hipLaunchKernelGGL(sa_mcadams_sums_kernel, dim3(nblk, B), dim3(MC_SUM_THREADS), 0, s, wav, alpha, n_valid, N, T,
                       (const float*)F, sums);
  hipLaunchKernelGGL(sa_mcadams_gain_kernel, dim3(B), dim3(64), 0, s, alpha, (const double*)sums, nblk, level, g,
                     gain);
  hipLaunchKernelGGL(sa_mcadams_apply_kernel, dim3(sa_div_up(N, MC_APPLY), B), dim3(256), 0, s, wav, alpha, n_valid,
                     N, T, (const float*)F, (const double*)g, out);
  return -(int)hipGetLastError();
}
