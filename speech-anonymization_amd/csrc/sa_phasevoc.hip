// Phase-vocoder resynthesis (ops.pv_synth, pitchnorm.py): the time stretch of section 15 with the
// input's own phases carried through it, instead of Griffin-Lim's reconstruction from random ones.  With theta the
// phase of R in turns (fp64), i_s the frame the stretch reads for output frame s and a_s its weight:
//   phi'[0] = theta[0],  phi'[t'] = theta[0] + sum_{s < t'} (theta[i_s + 1] - theta[i_s])  (mod 1)
//   C[t'] = S'[t'] (cospi(2 phi'), sinpi(2 phi')),  S' the caller's magnitudes or (1 - a) |R_i| + a |R_{i+1}|
// phi' is a prefix sum along t' per (row, bin): a chunked scan in three launches, lanes over the 201 bins so that a
// frame of R is one coalesced 1608-byte row.  No workgroup waits on another one; no atomics; every sum in a fixed
// order, the same bits on every run.
//   sa_pv_scan_kernel<false>  grid (chunks, B): the sum of a chunk's PV_TC increments, mod 1 -> ws[b][chunk][k]
//   sa_pv_offsets_kernel      grid (B): ws[b][chunk][k] <- phi' at the chunk's first frame (an exclusive scan)
//   sa_pv_scan_kernel<true>   grid (chunks, B): the increments again, from the offset on -> C (and phi')
// The increments are recomputed (two atan2 per element in all) rather than kept: [B][Tout][201] fp64 through HBM
// and back would cost more.
// sa_pv_synth_map is the same three launches with the stretch positions of a time map in place
// of a ratio's (MAP == true: sa_contour_map.h) and the magnitudes given on the input grid: one kernel text.
#include "sa_common.h"
#include "sa_pitch_shared.h"
#include "sa_contour_map.h"
#include <errno.h>

#define PV_TC 32                         // output frames per chunk
#define PV_THREADS 256                   // one thread per bin, 201 of them live
#define PV_TWO_PI 6.283185307179586476925286766559

extern "C" int sa_pv_dim(int which) {
  switch (which) {
    case 0: return 400;
    case 1: return 160;
    case 2: return PN_NBIN;
    case 3: return PV_TC;
    case 4: return PV_THREADS;
    default: return -EINVAL;
  }
}

static inline bool pv_shape_ok(int B, int Tout) { return B >= 1 && B <= PN_MAX_B && Tout >= 1 && Tout <= PN_MAX_T; }

extern "C" long long sa_pv_workspace_bytes(int B, int Tout) {
  if (!pv_shape_ok(B, Tout)) return -EINVAL;
  return 8LL * B * sa_div_up(Tout, PV_TC) * PN_NBIN;
}

__device__ static inline double pv_theta(float2 v) { return atan2((double)v.y, (double)v.x) / PV_TWO_PI; }

__device__ static inline double pv_mod1(double x) { return x - floor(x); }

// One chunk of one row.  i_s does not decrease with s, so the thread keeps the phase and the magnitude of the two
// frames it read last and computes only what is new (the branches are the same in every lane: i_s depends on the
// row and s alone).  SYNTH == false stops at T'_b and leaves the chunk's total; SYNTH == true starts from the
// chunk's offset and writes every frame of the chunk, zeros from T'_b on.
// MAP: S is on the input grid [B][T][201] (or NULL: |R|) and is mixed as the stretch mixes |R|; rq and Q are the
// row's tables, and the chunk finds its first i by a binary search over Q -- the same in every lane.
template <bool SYNTH, bool MAP>
__global__ __launch_bounds__(PV_THREADS) void sa_pv_scan_kernel(const float2* __restrict__ R,
                                                                const float* __restrict__ S,
                                                                const float* __restrict__ ratio,
                                                                const int* __restrict__ rq,
                                                                const long long* __restrict__ Q, int T, int Tout,
                                                                int nchunk, double* __restrict__ ws,
                                                                float2* __restrict__ C, double* __restrict__ phase) {
  const int k = threadIdx.x, c = blockIdx.x, b = blockIdx.y;
  if (k >= PN_NBIN) return;
  double r = 1.0;
  if constexpr (MAP) {
    rq += (size_t)b * T;
    Q += (size_t)b * T;
  } else {
    r = (double)pn_ratio(ratio[b]);
  }
  int Tb;
  if constexpr (MAP) Tb = ct_frames(Q, T); else Tb = pn_frames(T, r);
  const int t0 = c * PV_TC, t1 = min(t0 + PV_TC, Tout);
  if (!SYNTH && t0 >= Tb) return;                            // (a total nobody reads)
  const float2* Rb = R + (size_t)b * T * PN_NBIN + k;
  const float* Sb = MAP && S ? S + (size_t)b * T * PN_NBIN + k : nullptr;
  int i = 0;
  if constexpr (MAP) i = ct_search(Q, T, (long long)t0 << CT_QBITS);
  double* w = ws + ((size_t)b * nchunk + c) * PN_NBIN + k;
  double acc = SYNTH && t0 < Tb ? *w : 0.0;
  int cur = -2;                                              // the frames held: cur and cur + 1
  double th_lo = 0.0, th_hi = 0.0;
  float m_lo = 0.0f, m_hi = 0.0f;
  for (int tp = t0; tp < t1; ++tp) {
    const size_t o = ((size_t)b * Tout + tp) * PN_NBIN + k;
    if (tp >= Tb) {
      if (!SYNTH) break;
      C[o] = make_float2(0.0f, 0.0f);
      if (phase) phase[o] = 0.0;
      continue;
    }
    float a;
    if constexpr (MAP) i = ct_position(Q, rq, T, tp, i, &a); else i = pn_position(tp, r, T, &a);
    if (i != cur) {
      if (i == cur + 1) {
        th_lo = th_hi;
        m_lo = m_hi;
      } else {
        const float2 p = Rb[(size_t)i * PN_NBIN];
        th_lo = pv_theta(p);
        m_lo = Sb ? Sb[(size_t)i * PN_NBIN] : pn_mag(p);
      }
      const float2 q = Rb[(size_t)(i + 1) * PN_NBIN];
      th_hi = pv_theta(q);
      m_hi = Sb ? Sb[(size_t)(i + 1) * PN_NBIN] : pn_mag(q);
      cur = i;
    }
    if (SYNTH) {
      const double mag = (double)(!MAP && S ? S[o] : pn_mix(a, m_lo, m_hi));
      double sn, cs;
      sincospi(2.0 * acc, &sn, &cs);
      C[o] = make_float2((float)(mag * cs), (float)(mag * sn));
      if (phase) phase[o] = acc;
    }
    acc = pv_mod1(acc + (th_hi - th_lo));
  }
  if (!SYNTH) *w = acc;
}

// grid (B).  Thread k turns the totals of the chunks that start below T'_b into phi' at their first frames, in the
// order of the chunks, reduced mod 1 at every step.
template <bool MAP>
__global__ __launch_bounds__(PV_THREADS) void sa_pv_offsets_kernel(const float2* __restrict__ R,
                                                                   const float* __restrict__ ratio,
                                                                   const long long* __restrict__ Q, int T, int Tout,
                                                                   int nchunk, double* __restrict__ ws) {
  const int k = threadIdx.x, b = blockIdx.x;
  if (k >= PN_NBIN) return;
  int Tb;
  if constexpr (MAP) Tb = ct_frames(Q + (size_t)b * T, T); else Tb = pn_frames(T, (double)pn_ratio(ratio[b]));
  Tb = min(Tb, Tout);
  const int nuse = (Tb + PV_TC - 1) / PV_TC;                 // <= nchunk
  double* w = ws + (size_t)b * nchunk * PN_NBIN + k;
  double acc = pv_mod1(pv_theta(R[(size_t)b * T * PN_NBIN + k]));
  for (int c = 0; c < nuse; ++c) {
    const double tot = w[(size_t)c * PN_NBIN];
    w[(size_t)c * PN_NBIN] = acc;
    acc = pv_mod1(acc + tot);
  }
}

extern "C" int sa_pv_synth(const void* R, const float* S, const float* ratio, int B, int T, int Tout, void* C,
                           double* phase, void* ws, void* stream) {
  if (!R || !ratio || !C || !ws || !pv_shape_ok(B, Tout) || T < 2 || T > PN_MAX_T) return -EINVAL;
  const int nchunk = sa_div_up(Tout, PV_TC);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((sa_pv_scan_kernel<false, false>), dim3(nchunk, B), dim3(PV_THREADS), 0, st, (const float2*)R, S,
                     ratio, (const int*)nullptr, (const long long*)nullptr, T, Tout, nchunk, (double*)ws,
                     (float2*)nullptr, (double*)nullptr);
  hipLaunchKernelGGL(sa_pv_offsets_kernel<false>, dim3(B), dim3(PV_THREADS), 0, st, (const float2*)R, ratio,
                     (const long long*)nullptr, T, Tout, nchunk, (double*)ws);
  hipLaunchKernelGGL((sa_pv_scan_kernel<true, false>), dim3(nchunk, B), dim3(PV_THREADS), 0, st, (const float2*)R, S,
                     ratio, (const int*)nullptr, (const long long*)nullptr, T, Tout, nchunk, (double*)ws, (float2*)C,
                     phase);
  return -(int)hipGetLastError();
}

extern "C" int sa_pv_synth_map(const void* R, const float* M, const int* rho_q, const long long* Q, int B, int T,
                               int Tout, void* C, double* phase, void* ws, void* stream) {
  if (!R || !rho_q || !Q || !C || !ws || !pv_shape_ok(B, Tout) || T < 2 || T > PN_MAX_T) return -EINVAL;
  const int nchunk = sa_div_up(Tout, PV_TC);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((sa_pv_scan_kernel<false, true>), dim3(nchunk, B), dim3(PV_THREADS), 0, st, (const float2*)R, M,
                     (const float*)nullptr, rho_q, Q, T, Tout, nchunk, (double*)ws, (float2*)nullptr,
                     (double*)nullptr);
  hipLaunchKernelGGL(sa_pv_offsets_kernel<true>, dim3(B), dim3(PV_THREADS), 0, st, (const float2*)R,
                     (const float*)nullptr, Q, T, Tout, nchunk, (double*)ws);
  hipLaunchKernelGGL((sa_pv_scan_kernel<true, true>), dim3(nchunk, B), dim3(PV_THREADS), 0, st, (const float2*)R, M,
                     (const float*)nullptr, rho_q, Q, T, Tout, nchunk, (double*)ws, (float2*)C, phase);
  return -(int)hipGetLastError();
}
