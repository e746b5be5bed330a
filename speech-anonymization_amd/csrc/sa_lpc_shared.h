// The one text of what the LPC frame kernels share (DESIGN sections 17, 25, 26, 27).  One wave of 64 lanes per frame:
//   the fit         lag sums, silence test, Levinson-Durbin -- sa_lpc_fit, at any order, frame length and part length
//   the roots       Aberth-Ehrlich, one lane per root -- sa_lpc_aberth
//   the 320 frames  sqrt-Hann framing, all-pole recursion, frame store -- sa_fr_*, for sa_mcadams.hip,
//                   sa_formant_norm.hip and sa_srcfilt.hip; sa_fr_roots_kernel<M> is the frame kernel of the first two
//   the level       overlap-add gather, sums, gain and apply kernels and the host function that launches them --
//                   sa_fr_level<M>
//   the select      the key, inverse and workgroup count of the bitwise radix select of sa_formants.hip and
//                   sa_formant_norm.hip -- sa_sel_*
// M is what tells sa_mcadams from sa_pole_warp from sa_srcfilt_synth: M::COPIES says whether a row whose parameter is
// 1 is copied; where it is, M::clamp makes the row's parameter safe and M::angle maps a kept pole's angle.
// Every sum is in a fixed order and every multiply-add is an explicit fma: the bits depend on the text below, on the
// part lengths the callers pass (107 at order 20, 147 at order 18) and on nothing else.
#pragma once
#include "sa_common.h"
#include <errno.h>

#define SA_LPC_ITERS 64
#define SA_LPC_TOL2 1e-28                // (1e-14)^2
#define SA_LPC_SILENCE 1e-10
#define SA_LPC_REAL 1e-6                 // |Im z| <= 1e-6 |z|: a real root

#define SA_FR_W 320
#define SA_FR_H 160
#define SA_FR_P 20
#define SA_FR_PART 107                   // samples per part of a lag sum
#define SA_FR_G 1                        // frames per workgroup: one wave each
#define SA_FR_THREADS 64
#define SA_FR_CHUNK 4096                 // samples per block of the level sums
#define SA_FR_SUM_THREADS 256
#define SA_FR_APPLY 1024                 // samples per block of the last pass
#define SA_FR_MAX_B 65535                // grid.y
#define SA_FR_MAX_T (1 << 23)            // the vocoder's bound
#define SA_FR_MAX_N (1 << 30)            // sa_mcadams, sa_pole_warp; sa_srcfilt_synth takes 2^24

// ---- the fit -----------------------------------------------------------------------------------------
// r [P + 1] (r_0 already lifted) -> a [P + 1] with a_0 = 1 and err = r_0 prod (1 - k_i^2), the final prediction error;
// st = 2 when some |k_i| >= 1 or an error <= 0.  Fully unrolled: a and r stay in registers.  The status is set here:
// with the flag returned and tested by the caller instead, hipcc 7 scheduled sa_pole_warp_frame_kernel into 178 VGPRs
// against 114 (two waves per SIMD against four).
template <int P>
__device__ static __forceinline__ void sa_lpc_levinson(const double (&r)[P + 1], double (&a)[P + 1], int& st,
                                                       double& err_out) {
  double err = r[0];
  bool bad = false;
  a[0] = 1.0;
#pragma unroll
  for (int i = 1; i <= P; ++i) a[i] = 0.0;
#pragma unroll
  for (int m = 1; m <= P; ++m) {
    double acc = r[m];
#pragma unroll
    for (int i = 1; i < m; ++i) acc = fma(a[i], r[m - i], acc);
    const double k = -acc / err;
    bad = bad || !(fabs(k) < 1.0);
    double prev[P + 1];
#pragma unroll
    for (int i = 1; i < m; ++i) prev[i] = a[i];
#pragma unroll
    for (int i = 1; i < m; ++i) a[i] = fma(k, prev[m - i], prev[i]);
    a[m] = k;
    err *= 1.0 - k * k;
    bad = bad || !(err > 0.0);
  }
  err_out = err;
  if (bad) st = 2;
}

// The windowed frame f[0 .. W) at fs + OFF, with zeros up to f[W + P), and a barrier behind its stores -> the status
// (0, 1 silent, 2 no fit), and for status 0 the coefficients and the prediction error.  Lane (k, part) sums lag k over
// PART samples, the three parts are added in order; then every lane runs the recursion on the same values, so that
// the status is uniform and the coefficients are in every lane's registers.
template <int P, int W, int PART, int OFF>
__device__ static __forceinline__ int sa_lpc_fit(const double* fs, double* part, int lane, double (&a)[P + 1],
                                                 double& err) {
  {
    const int k = lane % (P + 1), p = min(lane / (P + 1), 2), j0 = PART * p, j1 = min(W, j0 + PART);
    double acc = 0.0;
    for (int j = j0; j < j1; ++j) acc = fma(fs[OFF + j], fs[OFF + j + k], acc);
    part[lane] = lane < 3 * (P + 1) ? acc : 0.0;
  }
  __syncthreads();
  double r[P + 1];
#pragma unroll
  for (int k = 0; k <= P; ++k) r[k] = (part[k] + part[P + 1 + k]) + part[2 * (P + 1) + k];
  int st = r[0] < SA_LPC_SILENCE ? 1 : 0;
  if (st == 0) {
    r[0] *= 1.0 + 1e-9;
    sa_lpc_levinson<P>(r, a, st, err);
  }
  return st;
}

// ---- the roots ---------------------------------------------------------------------------------------
// lane j < P owns root j of z^P + a_1 z^(P-1) + ... + a_P, from 0.9 exp(2 pi i (j + 0.25) / P): Horner for p and p',
// the Aberth sum over the other P - 1 by lane reads; at most 64 iterations, stop when every correction is under
// 1e-14.  -> converged (uniform); zr, zi: the lane's root (the idle lanes' values mean nothing)
template <int P>
__device__ static __forceinline__ bool sa_lpc_aberth(const double (&a)[P + 1], int lane, double& zr, double& zi) {
  const bool mine = lane < P;
  {
    double s, c;
    sincospi(((double)lane + 0.25) * (2.0 / P), &s, &c);
    zr = mine ? 0.9 * c : 2.0 + (double)lane;               // the idle lanes sit far away, apart from each other
    zi = mine ? 0.9 * s : 0.0;
  }
  bool conv = false;
  for (int it = 0; it < SA_LPC_ITERS && !conv; ++it) {
    double pr = 1.0, pi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
    for (int k = 1; k <= P; ++k) {
      const double tr = fma(dr, zr, fma(-di, zi, pr)), ti = fma(dr, zi, fma(di, zr, pi));
      dr = tr, di = ti;
      const double ur = fma(pr, zr, fma(-pi, zi, a[k])), ui = fma(pr, zi, pi * zr);
      pr = ur, pi = ui;
    }
    const double dm = 1.0 / fma(dr, dr, di * di);
    const double qr = fma(pr, dr, pi * di) * dm, qi = fma(pi, dr, -pr * di) * dm;          // p / p'
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const double er = zr - __shfl(zr, k, 64), ei = zi - __shfl(zi, k, 64);
      const double m = 1.0 / fma(er, er, ei * ei);
      if (k != lane) sr = fma(er, m, sr), si = fma(-ei, m, si);
    }
    const double gr = 1.0 - fma(qr, sr, -qi * si), gi = -fma(qr, si, qi * sr);              // 1 - (p / p') sum
    const double gm = 1.0 / fma(gr, gr, gi * gi);
    const double cr = fma(qr, gr, qi * gi) * gm, ci = fma(qi, gr, -qr * gi) * gm;
    zr -= cr, zi -= ci;
    conv = !__any(mine && !(fma(cr, cr, ci * ci) < SA_LPC_TOL2));
  }
  return conv;
}

// ---- the frames of 320 samples at hop 160 ------------------------------------------------------------
__device__ static inline int sa_fr_valid(const int* __restrict__ n_valid, int b, int N) {
  return min(max(n_valid[b], 0), N);
}

__device__ static inline double sa_fr_window(int j) { return sqrt(0.5 - 0.5 * cospi((double)j * (1.0 / 160.0))); }

// (a) lane j mod 64 windows five samples of frame t into fs [20 + 320 + 20], with zeros on either side (the FIR's
// history and the lag sums' far end read zeros instead of branching), and keeps their window values in wv.  EXC: the
// excitation is windowed beside it into es [320], and ee is the lane's five squares of it, summed in order.
template <bool EXC>
__device__ static __forceinline__ void sa_fr_load(const float* __restrict__ wav, const float* __restrict__ exc, int b,
                                                  int t, int N, int nv, int lane, double* fs, double* es,
                                                  double (&wv)[5], double& ee) {
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + 64 * i, n = SA_FR_H * t - SA_FR_H + j;
    const bool in = n >= 0 && n < nv;
    const double x = in ? (double)wav[(size_t)b * N + n] : 0.0;
    double e = 0.0;
    if constexpr (EXC) e = in ? (double)exc[(size_t)b * N + n] : 0.0;
    wv[i] = sa_fr_window(j);
    fs[SA_FR_P + j] = wv[i] * x;
    if constexpr (EXC) {
      const double we = wv[i] * e;
      es[j] = we;
      ee = fma(we, we, ee);
    }
  }
  if (lane < SA_FR_P) fs[lane] = 0.0, fs[SA_FR_P + SA_FR_W + lane] = 0.0;
  __syncthreads();
}

// The all-pole filter 1 / c over the 320 samples in(0), in(1), ... into ys: the same recursion in every lane, its
// 20-sample history a register ring, the input read by broadcast.
template <class In>
__device__ static __forceinline__ void sa_fr_allpole(const double (&c)[SA_FR_P + 1], In in, double* ys) {
  double h[SA_FR_P];
#pragma unroll
  for (int k = 0; k < SA_FR_P; ++k) h[k] = 0.0;
  for (int jb = 0; jb < SA_FR_W; jb += SA_FR_P) {
#pragma unroll
    for (int u = 0; u < SA_FR_P; ++u) {                     // h[(j - k) mod 20] is sample j - k
      double s = in(jb + u);
#pragma unroll
      for (int k = 1; k <= SA_FR_P; ++k) s = fma(-c[k], h[(u - k + SA_FR_P) % SA_FR_P], s);
      h[u] = s;
      ys[jb + u] = s;
    }
  }
}

// F_t = fp32(rec w): rec is the filtered frame (status 0), zeros (status 3, which only sa_srcfilt.hip gives) or the
// frame as it was
__device__ static __forceinline__ void sa_fr_store(float* __restrict__ F, int lane, int st, const double* ys,
                                                   const double* fs, const double (&wv)[5]) {
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + 64 * i;
    const double rec = st == 0 ? ys[j] : (st == 3 ? 0.0 : fs[SA_FR_P + j]);
    F[j] = (float)(rec * wv[i]);
  }
}

template <class M>
__device__ static inline bool sa_fr_copied(const float* __restrict__ par, int b) {
  if constexpr (M::COPIES) return M::clamp(par[b]) == 1.0;
  return false;
}

// The frame kernel that moves the roots (sa_mcadams, sa_pole_warp): grid (T, B), one wave.  LDS: the windowed frame
// between its zeros, the residual, the output.  ds_read_b64 (bank = (a / 4) mod 64, conflicts within a 32-lane half):
// the lanes of a wave read consecutive doubles (one 256-byte bank row per 32 lanes) or one address (a broadcast).  In
// (b) the lanes of a part read f[j] at one address and f[j + k] at 21 consecutive doubles; two parts share a half and
// lie 107 doubles = 11 mod 32 apart, so 10 of the second part's 11 doubles in the lower half fall on banks of the
// first: a two-way conflict on those reads, kept because the sums depend on the part length (section 25's 147-sample
// parts avoid it).
//   (a) lane j mod 64 windows five samples
//   (b) lane (k, part) sums lag k over a third of the frame; the three parts are added in order
//   (c) every lane runs the Levinson recursion on the same values (the coefficients are then in registers for d, f)
//   (d) lane j < 20 owns root j: Horner for p and p', the Aberth sum over the other 19 by lane reads
//   (e) lane i owns coefficient i of a' while the 20 factors are multiplied in, one per step
//   (f) FIR: five outputs per lane;  IIR: the 320-step recursion, the same in every lane
template <class M>
__global__ __launch_bounds__(SA_FR_THREADS) void sa_fr_roots_kernel(const float* __restrict__ wav,
                                                                    const float* __restrict__ par,
                                                                    const int* __restrict__ n_valid, int N, int T,
                                                                    float* __restrict__ ws,
                                                                    int* __restrict__ status) {
  __shared__ double fs[SA_FR_P + SA_FR_W + SA_FR_P];
  __shared__ double rs[SA_FR_W];
  __shared__ double ys[SA_FR_W];
  __shared__ double part[SA_FR_THREADS];
  __shared__ double a2s[SA_FR_P + 1];
  const int lane = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
  const double pb = M::clamp(par[b]);
  if (pb == 1.0) {                                          // the row is copied by the last pass; no frame is read
    if (status && lane == 0) status[(size_t)b * T + t] = 0;
    return;
  }
  double wv[5], a[SA_FR_P + 1], unused;
  // (a), (b), (c)
  sa_fr_load<false>(wav, nullptr, b, t, N, sa_fr_valid(n_valid, b, N), lane, fs, nullptr, wv, unused);
  int st = sa_lpc_fit<SA_FR_P, SA_FR_W, SA_FR_PART, SA_FR_P>(fs, part, lane, a, unused);

  if (st == 0) {
    // (d)
    const bool mine = lane < SA_FR_P;
    double zr, zi;
    const bool conv = sa_lpc_aberth<SA_FR_P>(a, lane, zr, zi);
    const double m2 = fma(zr, zr, zi * zi), mod = sqrt(m2);
    const bool real = mine && fabs(zi) <= SA_LPC_REAL * mod, up = mine && zi > SA_LPC_REAL * mod;
    const int nreal = __popcll(__ballot(real)), nup = __popcll(__ballot(up));
    if (!conv || 2 * nup + nreal != SA_FR_P) st = 2;

    if (st == 0) {
      // (e)
      double c1 = 0.0, c2 = 0.0;
      if (real) c1 = -zr;
      if (up) c1 = -2.0 * mod * cos(M::angle(atan2(zi, zr), pb)), c2 = m2;
      double p = lane == 0 ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < SA_FR_P; ++k) {
        const double k1 = __shfl(c1, k, 64), k2 = __shfl(c2, k, 64);
        const double u1 = __shfl_up(p, 1, 64), u2 = __shfl_up(p, 2, 64);
        p = fma(k2, lane >= 2 ? u2 : 0.0, fma(k1, lane >= 1 ? u1 : 0.0, p));
      }
      if (lane <= SA_FR_P) a2s[lane] = p;

      // (f)
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int j = lane + 64 * i;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k <= SA_FR_P; ++k) acc = fma(a[k], fs[SA_FR_P + j - k], acc);
        rs[j] = acc;
      }
    }
  }
  __syncthreads();
  if (st == 0) {
    double c[SA_FR_P + 1];
#pragma unroll
    for (int k = 1; k <= SA_FR_P; ++k) c[k] = a2s[k];
    sa_fr_allpole(c, [&](int j) { return rs[j]; }, ys);
  }
  __syncthreads();
  sa_fr_store(ws + ((size_t)b * T + t) * SA_FR_W, lane, st, ys, fs, wv);
  if (status && lane == 0) status[(size_t)b * T + t] = st;
}

// ---- overlap-add and level matching ------------------------------------------------------------------
// y[n] = F_t0[n - 160 t0 + 160] + F_{t0 + 1}[n - 160 t0], t0 = n / 160 (a gather)
__device__ static inline float sa_fr_y(const float* __restrict__ Fr, int n) {
  const int t0 = n / SA_FR_H, o = n - SA_FR_H * t0;
  return Fr[(size_t)t0 * SA_FR_W + o + SA_FR_H] + Fr[(size_t)(t0 + 1) * SA_FR_W + o];
}

// grid (blocks of 4096 samples, B): sums[b][blk] = (sum x^2, sum y^2) over the block's samples below n_valid, each
// thread its 16 samples in order, the wave by butterfly, the four waves in order; nothing for a copied row
template <class M>
__global__ __launch_bounds__(SA_FR_SUM_THREADS) void sa_fr_sums_kernel(const float* __restrict__ wav,
                                                                       const float* __restrict__ par,
                                                                       const int* __restrict__ n_valid, int N, int T,
                                                                       const float* __restrict__ ws,
                                                                       double* __restrict__ sums) {
  __shared__ double sh[2 * (SA_FR_SUM_THREADS / 64)];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (sa_fr_copied<M>(par, b)) return;
  const int nv = sa_fr_valid(n_valid, b, N);
  const float* Fr = ws + (size_t)b * T * SA_FR_W;
  double sx = 0.0, sy = 0.0;
  for (int i = 0; i < SA_FR_CHUNK / SA_FR_SUM_THREADS; ++i) {
    const int n = blockIdx.x * SA_FR_CHUNK + i * SA_FR_SUM_THREADS + tid;
    if (n < nv) {
      const double x = (double)wav[(size_t)b * N + n], y = (double)sa_fr_y(Fr, n);
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
// g = sqrt(sum x^2 / sum y^2), 1 when either is 0, when level is off, or when the row is copied
template <class M>
__global__ __launch_bounds__(64) void sa_fr_gain_kernel(const float* __restrict__ par,
                                                        const double* __restrict__ sums, int nblk, int level,
                                                        double* __restrict__ g, float* __restrict__ gain) {
  const int lane = threadIdx.x, b = blockIdx.x;
  double v = 1.0;
  if (level && !sa_fr_copied<M>(par, b)) {                  // (uniform)
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

// grid (blocks of 1024 samples, B): out = fp32(g y) below n_valid (the input itself in a copied row), 0 from there on
template <class M>
__global__ __launch_bounds__(256) void sa_fr_apply_kernel(const float* __restrict__ wav,
                                                          const float* __restrict__ par,
                                                          const int* __restrict__ n_valid, int N, int T,
                                                          const float* __restrict__ ws, const double* __restrict__ g,
                                                          float* __restrict__ out) {
  const int b = blockIdx.y;
  const bool copy = sa_fr_copied<M>(par, b);
  const int nv = sa_fr_valid(n_valid, b, N);
  const float* Fr = ws + (size_t)b * T * SA_FR_W;
  const double gb = g[b];
#pragma unroll
  for (int i = 0; i < SA_FR_APPLY / 256; ++i) {
    const int n = blockIdx.x * SA_FR_APPLY + i * 256 + threadIdx.x;
    if (n < N) {
      float v = 0.0f;
      if (n < nv) v = copy ? wav[(size_t)b * N + n] : (float)(gb * (double)sa_fr_y(Fr, n));
      out[(size_t)b * N + n] = v;
    }
  }
}

static inline int sa_fr_frames(int N) { return (N + SA_FR_H - 1) / SA_FR_H + 1; }

// The workspace is [B][T][320] fp32 frames, which the caller's frame kernel has been launched to fill, then the sums
// (fp64 [B][ceil(N / 4096)][2]) and the gains (fp64 [B]).  par is not read where M copies no rows.
template <class M>
static inline int sa_fr_level(const float* wav, const float* par, const int* n_valid, int B, int N, int level,
                              float* out, void* ws, float* gain, hipStream_t s) {
  const int T = sa_fr_frames(N), nblk = sa_div_up(N, SA_FR_CHUNK);
  const float* F = (const float*)ws;
  double* sums = (double*)(F + (size_t)B * T * SA_FR_W);    // 1280 bytes per frame: 8-byte aligned
  double* g = sums + 2 * (size_t)B * nblk;
  if (level)
    hipLaunchKernelGGL(sa_fr_sums_kernel<M>, dim3(nblk, B), dim3(SA_FR_SUM_THREADS), 0, s, wav, par, n_valid, N, T, F,
                       sums);
  hipLaunchKernelGGL(sa_fr_gain_kernel<M>, dim3(B), dim3(64), 0, s, par, (const double*)sums, nblk, level, g, gain);
  hipLaunchKernelGGL(sa_fr_apply_kernel<M>, dim3(sa_div_up(N, SA_FR_APPLY), B), dim3(256), 0, s, wav, par, n_valid, N,
                     T, F, (const double*)g, out);
  return -(int)hipGetLastError();
}

// sa_mcadams and sa_pole_warp from the first argument check to the last launch
template <class M>
static inline int sa_fr_roots(const float* wav, const float* par, const int* n_valid, int B, int N, int level,
                              float* out, void* ws, int* status, float* gain, void* stream) {
  if (!wav || !par || !n_valid || !out || !ws || B < 1 || B > SA_FR_MAX_B || N < 1 || N > SA_FR_MAX_N) return -EINVAL;
  const int T = sa_fr_frames(N);
  if (T > SA_FR_MAX_T) return -EINVAL;
  hipLaunchKernelGGL(sa_fr_roots_kernel<M>, dim3(T, B), dim3(SA_FR_THREADS), 0, (hipStream_t)stream, wav, par, n_valid,
                     N, T, (float*)ws, status);
  return sa_fr_level<M>(wav, par, n_valid, B, N, level, out, ws, gain, (hipStream_t)stream);
}

// ---- the bitwise radix select ------------------------------------------------------------------------
// a key whose unsigned order is the order of the fp32 values (any sign; the tracks' own values are positive)
__device__ static inline unsigned sa_sel_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ static inline float sa_sel_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ static inline int sa_sel_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The NC counts of every thread added over the workgroup: the wave by butterfly, the waves in order by every thread
// from LDS.  buf alternates between calls, so that one barrier per call is enough: a thread writes a buffer again only
// after the barrier of the call in between, which every thread reaches after its reads of that buffer.
template <int NC, int WAVES>
__device__ static inline void sa_sel_block_sum(int (&c)[NC], int (*cnt)[WAVES][NC], int buf) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NC; ++s) {
    const int v = sa_sel_wave_sum(c[s]);
    if (lane == 0) cnt[buf][wv][s] = v;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < NC; ++s) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) v += cnt[buf][w][s];
    c[s] = v;
  }
}
