// The LPC steps of the frame kernels, templated on the order P: the Levinson-Durbin recursion and the Aberth-Ehrlich
// root finder, as sa_mcadams.hip (P = 20) and sa_formants.hip (P = 18) each spell them out (DESIGN sections 17, 25).
// Included by sa_formant_norm.hip and sa_srcfilt.hip: the two older files keep their own copies, so that their objects
// stay what they were.  One wave of 64 lanes; every lane holds the same r and a.
#pragma once
#include "sa_common.h"

#define SA_LPC_ITERS 64
#define SA_LPC_TOL2 1e-28                // (1e-14)^2

// r [P + 1] (r_0 already lifted) -> a [P + 1] with a_0 = 1; st = 2 when some |k_i| >= 1 or an error <= 0.  Fully
// unrolled: a and r stay in registers.  The status is set here, as the older files do inline: with the flag returned
// and tested by the caller instead, hipcc 7 scheduled sa_pole_warp_frame_kernel into 178 VGPRs against 114 (two
// waves per SIMD against four).
template <int P>
__device__ static __forceinline__ void sa_lpc_levinson(const double (&r)[P + 1], double (&a)[P + 1], int& st) {
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
  if (bad) st = 2;
}

// The same recursion, word for word, which also hands out the final prediction error (err = r_0 prod (1 - k_i^2), formed
// step by step as above): sa_srcfilt.hip scales its excitation to it.  A second text and not a parameter of the first,
// so that sa_formant_norm.hip's object stays what it was.
template <int P>
__device__ static __forceinline__ void sa_lpc_levinson_err(const double (&r)[P + 1], double (&a)[P + 1], int& st,
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
