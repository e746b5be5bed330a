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
// The LPC and Aberth steps come from sa_lpc_shared.h at order 20; sa_mcadams.hip and sa_formants.hip keep their own.
// No atomics, every sum in a fixed order: the same bits on every run.
#include "sa_common.h"
#include "sa_lpc_shared.h"
#include <errno.h>

#define PW_W 320
#define PW_H 160
#define PW_P 20
#define PW_G 1                           // frames per workgroup: one wave each
#define PW_THREADS 64
#define PW_CHUNK 4096                    // samples per block of the level sums
#define PW_SUM_THREADS 256
#define PW_APPLY 1024                    // samples per block of the last pass
#define PW_MAX_B 65535                   // grid.y
#define PW_MAX_T (1 << 23)
#define PW_MAX_N (1 << 30)
#define PW_SILENCE 1e-10
#define PW_REAL 1e-6
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
    case 0: return PW_W;
    case 1: return PW_H;
    case 2: return PW_P;
    case 3: return PW_G;
    case 4: return PW_THREADS;
    case 5: return SA_LPC_ITERS;
    case 6: return PW_CHUNK;
    case 7: return PW_KNEE_PERMILLE;
    default: return -EINVAL;
  }
}

__device__ static inline double pw_q(float q) {             // a ratio no kernel can be led astray by
  return q >= 0.5f && q <= 2.0f ? (double)q : (q > 2.0f ? 2.0 : (q < 0.5f ? 0.5 : 1.0));
}

__device__ static inline double pw_angle(double phi, double q) {
  const double phi0 = (0.001 * PW_KNEE_PERMILLE * PW_PI) * fmin(1.0, 1.0 / q), low = q * phi0;
  return phi <= phi0 ? q * phi : low + (PW_PI - low) * ((phi - phi0) / (PW_PI - phi0));
}

__device__ static inline double pw_window(int j) { return sqrt(0.5 - 0.5 * cospi((double)j * (1.0 / 160.0))); }

// grid (T, B), one wave; the structure of sa_mcadams_frame_kernel.  LDS: the windowed frame with 20 zeros on either
// side (the FIR's history and the lag sums' far end read zeros instead of branching), the residual, the output.
// ds_read_b64 (bank = (a / 4) mod 64, conflicts within a 32-lane half): the lanes of a wave read consecutive doubles
// (one 256-byte bank row per 32 lanes) or one address (a broadcast).  In (b) the lanes of a part read f[j] at one
// address and f[j + k] at 21 consecutive doubles; two parts share a half and lie 107 doubles = 11 mod 32 apart, so
// 10 of the second part's 11 doubles in the lower half fall on banks of the first: a two-way conflict on those reads
// (sa_mcadams_frame_kernel's layout, kept so that the sums are its sums; section 25's 147-sample parts avoid it).
//   (a) lane j mod 64 windows five samples
//   (b) lane (k, part) sums lag k over a third of the frame; the three parts are added in order
//   (c) every lane runs the Levinson recursion on the same values, unrolled in registers
//   (d) lane j < 20 owns root j
//   (e) lane i owns coefficient i of a' while the 20 factors are multiplied in, one per step
//   (f) FIR: five outputs per lane;  IIR: the 320-step recursion, the same in every lane
__global__ __launch_bounds__(PW_THREADS) void sa_pole_warp_frame_kernel(const float* __restrict__ wav,
                                                                        const float* __restrict__ q,
                                                                        const int* __restrict__ n_valid, int N, int T,
                                                                        float* __restrict__ ws,
                                                                        int* __restrict__ status) {
  __shared__ double fs[PW_P + PW_W + PW_P];
  __shared__ double rs[PW_W];
  __shared__ double ys[PW_W];
  __shared__ double part[PW_THREADS];
  __shared__ double a2s[PW_P + 1];
  const int lane = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
  const double qb = pw_q(q[b]);
  if (qb == 1.0) {                                          // the row is copied by the last pass; no frame is read
    if (status && lane == 0) status[(size_t)b * T + t] = 0;
    return;
  }
  const int nv = min(max(n_valid[b], 0), N);
  float* F = ws + ((size_t)b * T + t) * PW_W;

  // (a)
  double wv[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + 64 * i, n = PW_H * t - PW_H + j;
    const double x = n >= 0 && n < nv ? (double)wav[(size_t)b * N + n] : 0.0;
    wv[i] = pw_window(j);
    fs[PW_P + j] = wv[i] * x;
  }
  if (lane < PW_P) fs[lane] = 0.0, fs[PW_P + PW_W + lane] = 0.0;
  __syncthreads();

  // (b)
  {
    const int k = lane % (PW_P + 1), p = min(lane / (PW_P + 1), 2), j0 = 107 * p, j1 = min(PW_W, j0 + 107);
    double acc = 0.0;
    for (int j = j0; j < j1; ++j) acc = fma(fs[PW_P + j], fs[PW_P + j + k], acc);
    part[lane] = lane < 3 * (PW_P + 1) ? acc : 0.0;
  }
  __syncthreads();
  double r[PW_P + 1];
#pragma unroll
  for (int k = 0; k <= PW_P; ++k) r[k] = (part[k] + part[PW_P + 1 + k]) + part[2 * (PW_P + 1) + k];

  int st = r[0] < PW_SILENCE ? 1 : 0;
  double a[PW_P + 1];
  if (st == 0) {                                            // (uniform: every lane holds the same r)
    // (c)
    r[0] *= 1.0 + 1e-9;
    sa_lpc_levinson<PW_P>(r, a, st);
  }

  if (st == 0) {
    // (d)
    const bool mine = lane < PW_P;
    double zr, zi;
    const bool conv = sa_lpc_aberth<PW_P>(a, lane, zr, zi);
    const double m2 = fma(zr, zr, zi * zi), mod = sqrt(m2);
    const bool real = mine && fabs(zi) <= PW_REAL * mod, up = mine && zi > PW_REAL * mod;
    const int nreal = __popcll(__ballot(real)), nup = __popcll(__ballot(up));
    if (!conv || 2 * nup + nreal != PW_P) st = 2;

    if (st == 0) {
      // (e)
      double c1 = 0.0, c2 = 0.0;
      if (real) c1 = -zr;
      if (up) c1 = -2.0 * mod * cos(pw_angle(atan2(zi, zr), qb)), c2 = m2;
      double p = lane == 0 ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < PW_P; ++k) {
        const double k1 = __shfl(c1, k, 64), k2 = __shfl(c2, k, 64);
        const double u1 = __shfl_up(p, 1, 64), u2 = __shfl_up(p, 2, 64);
        p = fma(k2, lane >= 2 ? u2 : 0.0, fma(k1, lane >= 1 ? u1 : 0.0, p));
      }
      if (lane <= PW_P) a2s[lane] = p;

      // (f)
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int j = lane + 64 * i;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k <= PW_P; ++k) acc = fma(a[k], fs[PW_P + j - k], acc);
        rs[j] = acc;
      }
    }
  }
  __syncthreads();
  if (st == 0) {
    double c[PW_P + 1], h[PW_P];
#pragma unroll
    for (int k = 1; k <= PW_P; ++k) c[k] = a2s[k], h[k - 1] = 0.0;
    for (int jb = 0; jb < PW_W; jb += PW_P) {
#pragma unroll
      for (int u = 0; u < PW_P; ++u) {                      // h[(j - k) mod 20] is sample j - k
        double s = rs[jb + u];
#pragma unroll
        for (int k = 1; k <= PW_P; ++k) s = fma(-c[k], h[(u - k + PW_P) % PW_P], s);
        h[u] = s;
        ys[jb + u] = s;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + 64 * i;
    F[j] = (float)((st == 0 ? ys[j] : fs[PW_P + j]) * wv[i]);
  }
  if (status && lane == 0) status[(size_t)b * T + t] = st;
}

__device__ static inline float pw_y(const float* __restrict__ Fr, int n) {
  const int t0 = n / PW_H, o = n - PW_H * t0;
  return Fr[(size_t)t0 * PW_W + o + PW_H] + Fr[(size_t)(t0 + 1) * PW_W + o];
}

// grid (blocks of 4096 samples, B): sums[b][blk] = (sum x^2, sum y^2) over the block's samples below n_valid, each
// thread its 16 samples in order, the wave by butterfly, the four waves in order
__global__ __launch_bounds__(PW_SUM_THREADS) void sa_pole_warp_sums_kernel(const float* __restrict__ wav,
                                                                           const float* __restrict__ q,
                                                                           const int* __restrict__ n_valid, int N,
                                                                           int T, const float* __restrict__ ws,
                                                                           double* __restrict__ sums) {
  __shared__ double sh[2 * (PW_SUM_THREADS / 64)];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (pw_q(q[b]) == 1.0) return;
  const int nv = min(max(n_valid[b], 0), N);
  const float* Fr = ws + (size_t)b * T * PW_W;
  double sx = 0.0, sy = 0.0;
  for (int i = 0; i < PW_CHUNK / PW_SUM_THREADS; ++i) {
    const int n = blockIdx.x * PW_CHUNK + i * PW_SUM_THREADS + tid;
    if (n < nv) {
      const double x = (double)wav[(size_t)b * N + n], y = (double)pw_y(Fr, n);
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
// g = sqrt(sum x^2 / sum y^2), 1 when either is 0, when level is off, or when q is 1
__global__ __launch_bounds__(64) void sa_pole_warp_gain_kernel(const float* __restrict__ q,
                                                               const double* __restrict__ sums, int nblk, int level,
                                                               double* __restrict__ g, float* __restrict__ gain) {
  const int lane = threadIdx.x, b = blockIdx.x;
  double v = 1.0;
  if (level && pw_q(q[b]) != 1.0) {                         // (uniform)
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

// grid (blocks of 1024 samples, B): out = fp32(g y) below n_valid (the input itself when q is 1), 0 from there on
__global__ __launch_bounds__(256) void sa_pole_warp_apply_kernel(const float* __restrict__ wav,
                                                                 const float* __restrict__ q,
                                                                 const int* __restrict__ n_valid, int N, int T,
                                                                 const float* __restrict__ ws,
                                                                 const double* __restrict__ g,
                                                                 float* __restrict__ out) {
  const int b = blockIdx.y;
  const bool copy = pw_q(q[b]) == 1.0;
  const int nv = min(max(n_valid[b], 0), N);
  const float* Fr = ws + (size_t)b * T * PW_W;
  const double gb = g[b];
#pragma unroll
  for (int i = 0; i < PW_APPLY / 256; ++i) {
    const int n = blockIdx.x * PW_APPLY + i * 256 + threadIdx.x;
    if (n < N) {
      float v = 0.0f;
      if (n < nv) v = copy ? wav[(size_t)b * N + n] : (float)(gb * (double)pw_y(Fr, n));
      out[(size_t)b * N + n] = v;
    }
  }
}

extern "C" int sa_pole_warp(const float* wav, const float* q, const int* n_valid, int B, int N, int level, float* out,
                            void* ws, int* status, float* gain, void* stream) {
  if (!wav || !q || !n_valid || !out || !ws || B < 1 || B > PW_MAX_B || N < 1 || N > PW_MAX_N) return -EINVAL;
  const int T = (N + PW_H - 1) / PW_H + 1;
  if (T > PW_MAX_T) return -EINVAL;
  const int nblk = sa_div_up(N, PW_CHUNK);
  float* F = (float*)ws;
  double* sums = (double*)(F + (size_t)B * T * PW_W);       // 1280 bytes per frame: 8-byte aligned
  double* g = sums + 2 * (size_t)B * nblk;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sa_pole_warp_frame_kernel, dim3(T, B), dim3(PW_THREADS), 0, s, wav, q, n_valid, N, T, F, status);
  if (level)
    hipLaunchKernelGGL(sa_pole_warp_sums_kernel, dim3(nblk, B), dim3(PW_SUM_THREADS), 0, s, wav, q, n_valid, N, T,
                       (const float*)F, sums);
  hipLaunchKernelGGL(sa_pole_warp_gain_kernel, dim3(B), dim3(64), 0, s, q, (const double*)sums, nblk, level, g, gain);
  hipLaunchKernelGGL(sa_pole_warp_apply_kernel, dim3(sa_div_up(N, PW_APPLY), B), dim3(256), 0, s, wav, q, n_valid, N,
                     T, (const float*)F, (const double*)g, out);
  return -(int)hipGetLastError();
}

// ---- the centre of a row's formants and the ratio to a target ---------------------------------------------
// a key whose unsigned order is the order of the fp32 values (a second copy of sa_formants.hip's)
__device__ static inline unsigned fn_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ static inline float fn_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ static inline int fn_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The three counts of every thread added over the workgroup: the wave by butterfly, the 16 waves in order by every
// thread from LDS.  buf alternates between calls, so that one barrier per call is enough: a thread writes a buffer
// again only after the barrier of the call in between, which every thread reaches after its reads of that buffer.
__device__ static inline void fn_block_sum(int (&c)[FN_NF], int (*cnt)[FN_WAVES][FN_NF], int buf) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < FN_NF; ++s) {
    const int v = fn_wave_sum_i(c[s]);
    if (lane == 0) cnt[buf][wv][s] = v;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < FN_NF; ++s) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < FN_WAVES; ++w) v += cnt[buf][w][s];
    c[s] = v;
  }
}

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
  fn_block_sum(c, cnt, 0);
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
          for (int k = 0; k < FN_NF; ++k) c[k] += (fn_key(Fr[(size_t)t * FN_NF + k]) & mask) == prefix[k];
        }
      }
      fn_block_sum(c, cnt, bit & 1);                        // (31 -> 1 after the count's 0, then alternating)
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
    const float m = scored ? fn_value(prefix[k]) : 0.0f;
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
  if (!freq || !status || !frames || !q || B < 1 || B > PW_MAX_B || T < 1 || T > FN_MAX_T || min_frames < 1)
    return -EINVAL;
  if (!(t1 >= FN_FMIN && t1 < t2 && t2 < t3 && t3 <= FN_FMAX)) return -EINVAL;
  if (!(q_min >= 0.5f && q_min <= 1.0f && q_max >= 1.0f && q_max <= 2.0f)) return -EINVAL;
  hipLaunchKernelGGL(sa_formant_centre_kernel, dim3(B), dim3(FN_THREADS), 0, (hipStream_t)stream, freq, status, f0,
                     frames, T, t1, t2, t3, q_min, q_max, min_frames, med, q, count);
  return -(int)hipGetLastError();
}
