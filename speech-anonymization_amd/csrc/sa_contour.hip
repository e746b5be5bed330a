// F0-contour pitch modification (pitchnorm.py): a ratio per frame instead of one per utterance,
// so that the output contour is target + gamma (f0 - mean) -- gamma 1 the additive shift of the reference's
// pitch-norm baseline, gamma 0 a monotone voice.  Two kernels here; sa_pv_synth_map (sa_phasevoc.hip) and
// sa_env_warp_frames (sa_envelope.hip) sit beside the siblings whose text they share.
//   sa_pitch_contour       f0 [B][T] -> rho_q [B][T] (the ratio in units of 2^-16), the time map Q [B][T] (int64,
//                          units of 2^-17 frames), T'_b, and sa_pitch_ratio's mean and voiced count
//   sa_pitch_resample_map  sa_pitch_resample with the read position taken from Q: integer arithmetic
// The time map is in integers so that no order of summation can change a bit of it.  Plain HIP, no atomics, fixed
// summation orders, the same bits on every run.
#include "sa_common.h"
#include "sa_pitch_shared.h"
#include "sa_contour_map.h"
#include <errno.h>

#define CT_W 256                         // frames per pass of sa_pitch_contour: the workgroup's width
#define CT_SMOOTH_MAX 8
#define CT_HALO CT_SMOOTH_MAX            // f^ a pass needs on either side of its frames
#define CT_FLOOR_HZ 60.0                 // YIN's lowest

extern "C" int sa_contour_dim(int which) {
  switch (which) {
    case 0: return CT_W;
    case 1: return CT_SMOOTH_MAX;
    case 2: return PN_HOP;
    case 3: return 16;                   // fraction bits of rho_q
    case 4: return CT_QBITS;             // fraction bits of Q
    case 5: return RS_TILE;
    case 6: return RS_SPAN;
    default: return -EINVAL;
  }
}

// ---- contour -----------------------------------------------------------------------------------------
// An inclusive scan over the workgroup's 256 threads in the order of the threads: shuffles within a wave, the four
// waves' totals through LDS.  *total: the fold of all 256.  Integers only, so the grouping cannot change a bit.
struct CtMax { __device__ static int op(int a, int b) { return max(a, b); } };
struct CtMin { __device__ static int op(int a, int b) { return min(a, b); } };
struct CtAdd { __device__ static long long op(long long a, long long b) { return a + b; } };

template <typename V, typename Op>
__device__ static inline V ct_scan(V v, V ident, V* sh, V* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V up = __shfl_up(v, o, 64);
    if (lane >= o) v = Op::op(up, v);
  }
  __syncthreads();                                            // (sh may still be read from the scan before)
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  V pre = ident, all = ident;
#pragma unroll
  for (int w = 0; w < CT_W / 64; ++w) {
    if (w < wave) pre = Op::op(pre, sh[w]);
    all = Op::op(all, sh[w]);
  }
  *total = all;
  return Op::op(pre, v);
}

// f^[t] of step 2 from the neighbours kept in Q's words by the passes A and B: l the last voiced frame <= t (-1:
// none), n the first one >= t (T: none).  The row has a voiced frame, so one of the two exists.
__device__ static inline double ct_fill(const float* __restrict__ f0, const long long* Qs, int T, int t) {
  const long long pk = Qs[t];
  const int l = (int)(pk >> 32), n = (int)(pk & 0xffffffffLL);
  if (l == t) return (double)f0[t];
  if (l < 0) return (double)f0[min(n, T - 1)];
  if (n >= T) return (double)f0[l];
  const double fl = (double)f0[l], fn = (double)f0[n];
  return fl + (fn - fl) * (double)(t - l) / (double)(n - l);
}

// grid (B): one workgroup of 256 threads per row, T walked in passes of 256 frames; no workgroup waits on another.
//   statistics  sa_pitch_ratio's, from the same text (pn_counted_frames and pn_voiced_mean, sa_pitch_shared.h)
//   pass A      l[t] by a max-scan of the voiced indices, left to right, with a carry between the passes
//   pass B      n[t] by a min-scan, right to left; (l, n) are kept in the words of Q, which nothing else needs yet
//   pass C      f^ of the tile and its halo into LDS, the triangle, the ratio, rho_q
//   pass D      Q by an int64 scan of w[t] = rho_q[t] + rho_q[t + 1] with a carry between the passes; T'_b
// A row under min_voiced voiced frames (or with none) skips A to C and gets rho_q = 2^16.
__global__ __launch_bounds__(CT_W) void sa_pitch_contour_kernel(const float* __restrict__ f0g,
                                                                const float* __restrict__ lens, int T, int N,
                                                                double target, double gamma, int smooth, double r_min,
                                                                double r_max, int min_voiced, int* rho_q,
                                                                long long* Qg, int* __restrict__ Tq,
                                                                float* __restrict__ mean, int* __restrict__ voiced) {
  __shared__ double stat[2];
  __shared__ int shi[4];
  __shared__ long long shl[4];
  __shared__ double fh[CT_W + 2 * CT_HALO];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* f0 = f0g + (size_t)b * T;
  int* rq = rho_q + (size_t)b * T;
  long long* Q = Qg + (size_t)b * T;

  const int F = pn_counted_frames(lens[b], N, T);
  int v0;
  const double m0 = pn_voiced_mean(f0, F, &v0);               // (thread 0's)
  if (tid == 0) {
    stat[0] = m0;
    stat[1] = (v0 >= min_voiced && m0 > 0.0) ? 1.0 : 0.0;
    mean[b] = (float)m0;
    voiced[b] = v0;
  }
  __syncthreads();
  const double m = stat[0];
  const bool moved = stat[1] != 0.0;                          // (the same in every thread)
  const int npass = (T + CT_W - 1) / CT_W;

  if (!moved) {
    for (int t = tid; t < T; t += CT_W) rq[t] = CT_RHO_ONE;
  } else {
    int carry = -1;                                           // pass A
    for (int p = 0; p < npass; ++p) {
      const int t = p * CT_W + tid;
      const int mine = (t < F && f0[t] > 0.0f) ? t : -1;
      int tot;
      const int l = max(carry, ct_scan<int, CtMax>(mine, -1, shi, &tot));
      if (t < T) Q[t] = (long long)((unsigned long long)(unsigned)l << 32);
      carry = max(carry, tot);
    }
    __syncthreads();                                          // (pass B completes the words other threads wrote)
    carry = T;                                                // pass B: thread tid takes the tile's frame 255 - tid
    for (int p = npass - 1; p >= 0; --p) {
      const int t = p * CT_W + (CT_W - 1 - tid);
      const int mine = (t < F && f0[t] > 0.0f) ? t : T;
      int tot;
      const int nx = min(carry, ct_scan<int, CtMin>(mine, T, shi, &tot));
      if (t < T) Q[t] = (Q[t] & ~0xffffffffLL) | (long long)nx;
      carry = min(carry, tot);
    }
    const double norm = (double)((smooth + 1) * (smooth + 1));
    for (int p = 0; p < npass; ++p) {                         // pass C
      const int t0 = p * CT_W;
      __syncthreads();                                        // (the words other threads wrote; fh of the pass before)
      for (int j = tid; j < CT_W + 2 * CT_HALO; j += CT_W)
        fh[j] = ct_fill(f0, Q, T, min(max(t0 - CT_HALO + j, 0), T - 1));
      __syncthreads();
      const int t = t0 + tid;
      if (t < T) {
        // f~[t]: frame clamp(t + j) sits at fh[clamp(t + j) - t0 + CT_HALO]
        double s = 0.0;
        for (int j = -smooth; j <= smooth; ++j) {
          const int u = min(max(t + j, 0), T - 1);
          s += (double)(smooth + 1 - abs(j)) * fh[u - t0 + CT_HALO];
        }
        const double fs = s / norm;
        const double g = fmax(CT_FLOOR_HZ, target + gamma * (fs - m));
        const double rho = fmin(fmax(g / fs, r_min), r_max);
        rq[t] = ct_rho((int)rint(rho * 65536.0));
      }
    }
  }
  __syncthreads();                                            // (pass D reads rho_q across threads)

  long long qc = 0;                                           // pass D
  for (int p = 0; p < npass; ++p) {
    const int t = p * CT_W + tid;
    const long long w = t <= T - 2 ? ct_w(rq, t) : 0LL;
    long long tot;
    const long long incl = ct_scan<long long, CtAdd>(w, 0LL, shl, &tot);
    if (t < T) {
      const long long q = qc + incl - w;
      Q[t] = q;
      if (t == T - 1) Tq[b] = (int)((q + CT_QONE - 1) >> CT_QBITS) + 1;
    }
    qc += tot;
  }
}

extern "C" int sa_pitch_contour(const float* f0, const float* lens, int B, int T, int N, float target, float gamma,
                                int smooth, float r_min, float r_max, int min_voiced, int* rho_q, long long* Q,
                                int* Tq, float* mean, int* voiced, void* stream) {
  if (!f0 || !lens || !rho_q || !Q || !Tq || !mean || !voiced || !pn_rows_ok(B) || !pn_frames_ok(T, 2) ||
      !pn_samples_ok(N) || !(target > 0.0f) || !(gamma >= 0.0f) || !(gamma <= 2.0f) || smooth < 0 ||
      smooth > CT_SMOOTH_MAX || !(r_min >= 0.5f) || !(r_max <= 2.0f) || !(r_min <= r_max))
    return -EINVAL;
  hipLaunchKernelGGL(sa_pitch_contour_kernel, dim3(B), dim3(CT_W), 0, (hipStream_t)stream, f0, lens, T, N,
                     (double)target, (double)gamma, smooth, (double)r_min, (double)r_max, min_voiced, rho_q, Q, Tq,
                     mean, voiced);
  return -(int)hipGetLastError();
}

// ---- resample ----------------------------------------------------------------------------------------
// grid (tiles of 256 outputs, B): sa_pitch_resample with the read position of output sample n taken from the time
// map.  With t = min(n / 160, T - 2) and u = n - 160 t:  Z = 160 Q[t] + w[t] u (int64), the position is Z / 2^17 =
// ip + fr, and the filter is section 15's at the local ratio r_loc = w[t] / 2^17 <= 2: c = min(1, 1 / r_loc),
// H = 16 / c <= 32, at most 64 taps.  Row b's input ends at (T'_b - 1) 160 samples, at most Nin.  The workgroup
// stages the span [ip(n0) - 32, ip(n0) - 32 + 578): the positions of a tile advance by at most 2 per sample, so every
// tap of the tile lies inside (a tap that does not -- a table no sa_pitch_contour wrote -- is left out).  The taps
// are sa_pitch_resample's loop (pn_rs_taps, sa_pitch_shared.h) at the position ip + fr and the ratio r_loc.
__device__ static inline long long ctr_position(const int* __restrict__ rq, const long long* __restrict__ Q, int T,
                                                int n, long long* w) {
  const int t = min(n / PN_HOP, T - 2);
  *w = ct_w(rq, t);
  const long long q = min(max(Q[t], 0LL), (long long)t << 18);
  return (long long)PN_HOP * q + *w * (long long)(n - PN_HOP * t);
}

__global__ __launch_bounds__(RS_TILE) void sa_pitch_resample_map_kernel(const float* __restrict__ y,
                                                                        const int* __restrict__ rho_q,
                                                                        const long long* __restrict__ Qg,
                                                                        const int* __restrict__ n_valid, int Nin,
                                                                        int Nout, int T, float* __restrict__ out) {
  __shared__ float ys[RS_SPAN];
  const int tid = threadIdx.x, b = blockIdx.y, n0 = blockIdx.x * RS_TILE, n = n0 + tid;
  const int* rq = rho_q + (size_t)b * T;
  const long long* Q = Qg + (size_t)b * T;
  const long long vin = min((long long)Nin, (long long)PN_HOP * (long long)(ct_frames(Q, T) - 1));
  long long w;
  const long long span0 = (ctr_position(rq, Q, T, n0, &w) >> CT_QBITS) - 32;
  for (int i = tid; i < RS_SPAN; i += RS_TILE) {
    const long long s = span0 + i;
    ys[i] = (s >= 0 && s < vin) ? y[(size_t)b * Nin + s] : 0.0f;
  }
  __syncthreads();
  if (n >= Nout) return;
  float acc = 0.0f;
  if (n < n_valid[b]) {
    const long long Z = ctr_position(rq, Q, T, n, &w);
    const long long ip = Z >> CT_QBITS;
    const double fr = (double)(Z & (CT_QONE - 1)) * (1.0 / (double)CT_QONE);
    acc = pn_rs_taps<true>(ys, span0, (double)ip + fr, (double)w * (1.0 / (double)CT_QONE));
  }
  out[(size_t)b * Nout + n] = acc;
}

extern "C" int sa_pitch_resample_map(const float* y, const int* rho_q, const long long* Q, const int* n_valid, int B,
                                     int Nin, int Nout, int T, float* out, void* stream) {
  if (!y || !rho_q || !Q || !n_valid || !out || !pn_rows_ok(B) || !pn_samples_ok(Nin) || Nout < 1 ||
      Nout > PN_MAX_N / 2 || !pn_frames_ok(T, 2))
    return -EINVAL;
  hipLaunchKernelGGL(sa_pitch_resample_map_kernel, dim3(sa_div_up(Nout, RS_TILE), B), dim3(RS_TILE), 0,
                     (hipStream_t)stream, y, rho_q, Q, n_valid, Nin, Nout, T, out);
  return -(int)hipGetLastError();
}
