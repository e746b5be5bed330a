// LPC source-filter resynthesis (sourcefilter.py; ops.srcfilt_pulses, ops.srcfilt_excite, ops.srcfilt_synth; DESIGN
// section 27; include/sa_hip.h carries the definition).  The classic LPC vocoder: every frame keeps its all-pole
// envelope and its energy, the residual is thrown away, and the filter is driven by a synthetic excitation -- pulses at
// the F0 track where the frame is voiced, noise elsewhere.  The pulses are laid down at whatever period is asked for, so
// the same pass moves the pitch.
//   sa_srcfilt_pulses   f0, rho_q -> where every pulse goes (pos_q, int64 in units of 2^-16 samples) and its period
//   sa_srcfilt_excite   the pulse table -> the excitation: hashed uniform noise plus the linearly interpolated pulses
//   sa_srcfilt_synth    sa_mcadams's framing, fit, overlap-add and level matching; the frame is the
//                       all-pole filter 1 / a driven by the windowed excitation, scaled to the frame's prediction error
// Every decision of the first two is made on integers, or on fp64 formed from the fp32 inputs; the excitation's fp32
// operations are rounded one by one.  Only the filtered output has a rounding bar.  No root finder, no FIR.
// Plain HIP C++, no atomics, fixed summation orders: the same bits on every run, and a row alone gives the bits it
// gives inside a batch.
#include "sa_common.h"
#include "sa_lpc_shared.h"
#include <errno.h>
#include <limits.h>
#include <math.h>

#define SF_W 320
#define SF_H 160
#define SF_P 20
#define SF_THREADS 64
#define SF_CHUNK 4096                    // samples per block of the level sums
#define SF_SUM_THREADS 256
#define SF_APPLY 1024                    // samples per block of the last pass
#define SF_MAX_B 65535                   // grid.y
#define SF_MAX_N (1 << 24)
#define SF_SILENCE 1e-10
#define SF_NO_EXC 1e-20
#define SF_TMIN 40                       // the period's bounds in samples: 400 Hz ..
#define SF_TMAX 266                      // .. 60 Hz
#define SF_KDIV 40                       // Kcap = N / 40 + 2
#define SF_FCHUNK 1024                   // frames whose periods the pulse walk stages at a time
#define SF_TILE 256                      // samples per workgroup of sa_srcfilt_excite
#define SF_G 8                           // pulses staged per tile: (256 + 1) / 40 + 1 = 7 can touch one
#define SF_ONE (1 << 16)
#define SF_NUM 68719476736000.0          // 16000 2^32

extern "C" int sa_srcfilt_dim(int which) {
  switch (which) {
    case 0: return SF_W;
    case 1: return SF_H;
    case 2: return SF_P;
    case 3: return SF_THREADS;
    case 4: return SF_CHUNK;
    case 5: return SF_TMIN;
    case 6: return SF_TMAX;
    case 7: return SF_KDIV;
    case 8: return SF_TILE;
    case 9: return SF_G;
    default: return -EINVAL;
  }
}

static inline bool sf_dims_ok(int B, int N) { return B >= 1 && B <= SF_MAX_B && N >= 1 && N <= SF_MAX_N; }
static inline bool sf_frames_ok(int N, int T) { return T == N / SF_H + 1 || T == (N + SF_H - 1) / SF_H + 1; }
static inline int sf_synth_frames(int N) { return (N + SF_H - 1) / SF_H + 1; }

extern "C" long long sa_srcfilt_workspace_bytes(int B, int N) {
  if (!sf_dims_ok(B, N)) return -EINVAL;
  return 4LL * B * sf_synth_frames(N) * SF_W + 8LL * (2LL * B * sa_div_up(N, SF_CHUNK) + B);
}

__device__ static inline int sf_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ static inline int sf_frame(int n, int T) { return min((n + SF_H / 2) / SF_H, T - 1); }
__device__ static inline bool sf_voiced(float f) { return f > 0.0f && f < INFINITY; }       // (a NaN is unvoiced)

// P_q[t]: the period of frame t in units of 2^-16 samples, 0 where it is unvoiced.  The product of a 24-bit and an
// 18-bit number is exact in fp64; the quotient is rounded once; the clamp comes before the conversion.
__device__ static inline int sf_period(const float* __restrict__ f0, const int* __restrict__ rq, int t) {
  const float f = f0[t];
  if (!sf_voiced(f)) return 0;
  const int rho = rq ? sf_clamp(rq[t], SF_ONE / 2, 2 * SF_ONE) : SF_ONE;
  const double p = rint(SF_NUM / ((double)f * (double)rho));
  return (int)fmin(fmax(p, (double)SF_TMIN * SF_ONE), (double)SF_TMAX * SF_ONE);
}

// ---- pulses ------------------------------------------------------------------------------------------
// grid (B), one wave per row, as sa_psola_plan.  The lanes form the periods of SF_FCHUNK frames at a time into LDS, so
// that the fp64 division is off the chain; then every lane walks the chain (the same walk in each) and lane 0 writes.
// The period is read from LDS only when the position leaves its frame, and made a scalar there: between two frames a
// step is a scalar add and two compares (0.286 ms at 32 x 10 s against 0.333 ms with a read per step).  A step either
// emits a pulse and advances by 40 samples or more, or jumps to the first sample of the next frame, or ends the row:
// s grows with every step, so the walk ends after at most Kcap + T of them.
__global__ __launch_bounds__(SF_THREADS) void sa_srcfilt_pulses_kernel(const float* __restrict__ f0g,
                                                                       const int* __restrict__ rho_q,
                                                                       const int* __restrict__ n_valid, int N, int T,
                                                                       int Kcap, long long* __restrict__ pos_q,
                                                                       int* __restrict__ period_q,
                                                                       int* __restrict__ count) {
  __shared__ int ps[SF_FCHUNK];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = sf_clamp(n_valid[b], 0, N);
  const float* f0 = f0g + (size_t)b * T;
  const int* rq = rho_q ? rho_q + (size_t)b * T : nullptr;
  long long* pq = pos_q + (size_t)b * Kcap;
  int* dq = period_q + (size_t)b * Kcap;

  const long long end = (long long)nv << 16;
  long long s = 0, next = 0;                                // next: where the frame has to be looked up again
  int fb = -1, k = 0, t = 0, p = 0;
  for (int step = 0; step < Kcap + T && s < end && k < Kcap; ++step) {        // (uniform)
    if (s >= next) {                                        // floor(s / 2^16) has left frame t: the LDS read is off the
      t = sf_frame((int)(s >> 16), T);                      // chain for the other pulses of a frame
      if (fb < 0 || t >= fb + SF_FCHUNK) {
        __syncthreads();
        fb = t;
        for (int i = lane; i < SF_FCHUNK; i += SF_THREADS) ps[i] = fb + i < T ? sf_period(f0, rq, fb + i) : 0;
        __syncthreads();
      }
      p = __builtin_amdgcn_readfirstlane(ps[t - fb]);       // (the same in every lane: a scalar from here on)
      next = t == T - 1 ? LLONG_MAX : (long long)(SF_H * t + SF_H / 2) << 16;
    }
    if (p > 0) {
      if (lane == 0) pq[k] = s, dq[k] = p;
      ++k;
      s += p;
    } else if (t == T - 1) {
      break;
    } else {
      s = next;
    }
  }
  if (lane == 0) count[b] = k;
}

extern "C" int sa_srcfilt_pulses(const float* f0, const int* rho_q, const int* n_valid, int B, int N, int T,
                                 long long* pos_q, int* period_q, int* count, void* stream) {
  if (!f0 || !n_valid || !pos_q || !period_q || !count || !sf_dims_ok(B, N) || !sf_frames_ok(N, T)) return -EINVAL;
  hipLaunchKernelGGL(sa_srcfilt_pulses_kernel, dim3(B), dim3(SF_THREADS), 0, (hipStream_t)stream, f0, rho_q, n_valid,
                     N, T, N / SF_KDIV + 2, pos_q, period_q, count);
  return -(int)hipGetLastError();
}

// ---- excitation --------------------------------------------------------------------------------------
__device__ static inline unsigned sf_mix(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// grid (ceil(N / 256), B).  A pulse touches the tile [n0, n0 + 256) when its integer position lies in
// [n0 - 1, n0 + 255]: at a spacing of 40 or more that is 7 pulses at the most.  The first SF_G threads each find the
// first of them by the same binary search and stage one; every thread then looks through the staged ones.  What is
// read from the tables is only compared or clamped: a table no kernel wrote changes values, never addresses.
__global__ __launch_bounds__(SF_TILE) void sa_srcfilt_excite_kernel(const float* __restrict__ f0g,
                                                                    const long long* __restrict__ pos_q,
                                                                    const int* __restrict__ period_q,
                                                                    const int* __restrict__ count,
                                                                    const int* __restrict__ seed,
                                                                    const int* __restrict__ n_valid, int N, int T,
                                                                    int Kcap, float aspiration,
                                                                    float* __restrict__ exc) {
  __shared__ long long sp[SF_G];
  __shared__ float sa[SF_G];
  const int tid = threadIdx.x, b = blockIdx.y, n0 = blockIdx.x * SF_TILE, n = n0 + tid;
  const int nv = sf_clamp(n_valid[b], 0, N);
  if (tid < SF_G) {
    const int cnt = sf_clamp(count[b], 0, Kcap);
    const long long* pq = pos_q + (size_t)b * Kcap;
    const long long first = (long long)max(n0 - 1, 0) << 16;
    int lo = 0, hi = cnt;                                     // the first entry at or past ``first``
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (pq[mid] < first) lo = mid + 1; else hi = mid;
    }
    const int k = lo + tid;
    long long s = -1;
    float A = 0.0f;
    if (k < cnt) {
      s = pq[k];
      const int p = sf_clamp(period_q[(size_t)b * Kcap + k], SF_TMIN * SF_ONE, SF_TMAX * SF_ONE);
      A = (float)sqrt((double)p * (1.0 / SF_ONE));
    }
    sp[tid] = s;
    sa[tid] = A;
  }
  __syncthreads();
  if (n >= N) return;
  float e = 0.0f;
  if (n < nv) {
    // every product and sum below is rounded on its own: the pragma keeps the compiler from fusing them (the
    // __fmul_rn / __fadd_rn of this toolchain are the plain operators, which the default contraction would fuse)
#pragma clang fp contract(off)
    const unsigned h = sf_mix((unsigned)n ^ sf_mix((unsigned)seed[b]));
    const float u = (float)((int)(h >> 8) - (1 << 23)) * (1.0f / (1 << 23));
    const float c = sf_voiced(f0g[(size_t)b * T + sf_frame(n, T)]) ? aspiration : 1.0f;
    e = c * u;
#pragma unroll
    for (int i = 0; i < SF_G; ++i) {
      const long long s = sp[i];
      if (s < 0) continue;
      const long long m = s >> 16;
      const int frac = (int)(s & (SF_ONE - 1));
      const float phi = (float)frac * (1.0f / SF_ONE);
      if (m == (long long)n) {
        const float term = sa[i] * (1.0f - phi);
        e = e + term;
      } else if (m + 1 == (long long)n && frac > 0) {
        const float term = sa[i] * phi;
        e = e + term;
      }
    }
  }
  exc[(size_t)b * N + n] = e;
}

extern "C" int sa_srcfilt_excite(const float* f0, const long long* pos_q, const int* period_q, const int* count,
                                 const int* seed, const int* n_valid, int B, int N, int T, float aspiration,
                                 float* exc, void* stream) {
  if (!f0 || !pos_q || !period_q || !count || !seed || !n_valid || !exc || !sf_dims_ok(B, N) || !sf_frames_ok(N, T))
    return -EINVAL;
  if (!(aspiration >= 0.0f && aspiration <= 1.0f)) return -EINVAL;         // (a NaN too)
  hipLaunchKernelGGL(sa_srcfilt_excite_kernel, dim3(sa_div_up(N, SF_TILE), B), dim3(SF_TILE), 0, (hipStream_t)stream,
                     f0, pos_q, period_q, count, seed, n_valid, N, T, N / SF_KDIV + 2, aspiration, exc);
  return -(int)hipGetLastError();
}

// ---- synthesis ---------------------------------------------------------------------------------------
__device__ static inline double sf_window(int j) { return sqrt(0.5 - 0.5 * cospi((double)j * (1.0 / 160.0))); }

// grid (T, B), one wave; the structure of sa_pole_warp_frame_kernel without its roots and its FIR.  LDS: the windowed
// frame with 20 zeros on either side (the lag sums' far end reads zeros instead of branching), the windowed
// excitation, the output.
//   (a) lane j mod 64 windows five samples of the frame and of the excitation
//   (b) lane (k, part) sums lag k over a third of the frame; the three parts are added in order: sa_mcadams's sums
//   (c) every lane runs the Levinson recursion on the same values, unrolled in registers
//   (d) Ee: five squares per lane in order, the wave by butterfly
//   (e) IIR: the 320-step recursion on g ex, the same in every lane, its history a register ring
__global__ __launch_bounds__(SF_THREADS) void sa_srcfilt_frame_kernel(const float* __restrict__ wav,
                                                                      const float* __restrict__ exc,
                                                                      const int* __restrict__ n_valid, int N, int T,
                                                                      float* __restrict__ ws,
                                                                      int* __restrict__ status) {
  __shared__ double fs[SF_P + SF_W + SF_P];
  __shared__ double es[SF_W];
  __shared__ double ys[SF_W];
  __shared__ double part[SF_THREADS];
  const int lane = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
  const int nv = sf_clamp(n_valid[b], 0, N);
  float* F = ws + ((size_t)b * T + t) * SF_W;

  // (a)
  double wv[5], ee = 0.0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + 64 * i, n = SF_H * t - SF_H + j;
    const bool in = n >= 0 && n < nv;
    const double x = in ? (double)wav[(size_t)b * N + n] : 0.0;
    const double e = in ? (double)exc[(size_t)b * N + n] : 0.0;
    wv[i] = sf_window(j);
    fs[SF_P + j] = wv[i] * x;
    const double we = wv[i] * e;
    es[j] = we;
    ee = fma(we, we, ee);
  }
  if (lane < SF_P) fs[lane] = 0.0, fs[SF_P + SF_W + lane] = 0.0;
  __syncthreads();

  // (b)
  {
    const int k = lane % (SF_P + 1), p = min(lane / (SF_P + 1), 2), j0 = 107 * p, j1 = min(SF_W, j0 + 107);
    double acc = 0.0;
    for (int j = j0; j < j1; ++j) acc = fma(fs[SF_P + j], fs[SF_P + j + k], acc);
    part[lane] = lane < 3 * (SF_P + 1) ? acc : 0.0;
  }
  __syncthreads();
  double r[SF_P + 1];
#pragma unroll
  for (int k = 0; k <= SF_P; ++k) r[k] = (part[k] + part[SF_P + 1 + k]) + part[2 * (SF_P + 1) + k];

  int st = r[0] < SF_SILENCE ? 1 : 0;
  double a[SF_P + 1], err = 0.0;
  if (st == 0) {                                            // (uniform: every lane holds the same r)
    // (c)
    r[0] *= 1.0 + 1e-9;
    sa_lpc_levinson_err<SF_P>(r, a, st, err);
  }
  // (d)
  ee = sa_wave_sum_d(ee);
  if (st == 0 && ee < SF_NO_EXC) st = 3;

  if (st == 0) {
    // (e)
    const double g = sqrt(err / ee);
    double h[SF_P];
#pragma unroll
    for (int k = 0; k < SF_P; ++k) h[k] = 0.0;
    for (int jb = 0; jb < SF_W; jb += SF_P) {
#pragma unroll
      for (int u = 0; u < SF_P; ++u) {                      // h[(j - k) mod 20] is sample j - k
        double s = g * es[jb + u];
#pragma unroll
        for (int k = 1; k <= SF_P; ++k) s = fma(-a[k], h[(u - k + SF_P) % SF_P], s);
        h[u] = s;
        ys[jb + u] = s;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + 64 * i;
    const double rec = st == 0 ? ys[j] : (st == 3 ? 0.0 : fs[SF_P + j]);
    F[j] = (float)(rec * wv[i]);
  }
  if (status && lane == 0) status[(size_t)b * T + t] = st;
}

__device__ static inline float sf_y(const float* __restrict__ Fr, int n) {
  const int t0 = n / SF_H, o = n - SF_H * t0;
  return Fr[(size_t)t0 * SF_W + o + SF_H] + Fr[(size_t)(t0 + 1) * SF_W + o];
}

// grid (blocks of 4096 samples, B): sums[b][blk] = (sum x^2, sum y^2) over the block's samples below n_valid, each
// thread its 16 samples in order, the wave by butterfly, the four waves in order (sa_mcadams's pass)
__global__ __launch_bounds__(SF_SUM_THREADS) void sa_srcfilt_sums_kernel(const float* __restrict__ wav,
                                                                         const int* __restrict__ n_valid, int N, int T,
                                                                         const float* __restrict__ ws,
                                                                         double* __restrict__ sums) {
  __shared__ double sh[2 * (SF_SUM_THREADS / 64)];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int nv = sf_clamp(n_valid[b], 0, N);
  const float* Fr = ws + (size_t)b * T * SF_W;
  double sx = 0.0, sy = 0.0;
  for (int i = 0; i < SF_CHUNK / SF_SUM_THREADS; ++i) {
    const int n = blockIdx.x * SF_CHUNK + i * SF_SUM_THREADS + tid;
    if (n < nv) {
      const double x = (double)wav[(size_t)b * N + n], y = (double)sf_y(Fr, n);
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
// g = sqrt(sum x^2 / sum y^2), 1 when either is 0 or when level is off
__global__ __launch_bounds__(64) void sa_srcfilt_gain_kernel(const double* __restrict__ sums, int nblk, int level,
                                                             double* __restrict__ g, float* __restrict__ gain) {
  const int lane = threadIdx.x, b = blockIdx.x;
  double v = 1.0;
  if (level) {
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

// grid (blocks of 1024 samples, B): out = fp32(g y) below n_valid, 0 from there on
__global__ __launch_bounds__(256) void sa_srcfilt_apply_kernel(const int* __restrict__ n_valid, int N, int T,
                                                               const float* __restrict__ ws,
                                                               const double* __restrict__ g,
                                                               float* __restrict__ out) {
  const int b = blockIdx.y;
  const int nv = sf_clamp(n_valid[b], 0, N);
  const float* Fr = ws + (size_t)b * T * SF_W;
  const double gb = g[b];
#pragma unroll
  for (int i = 0; i < SF_APPLY / 256; ++i) {
    const int n = blockIdx.x * SF_APPLY + i * 256 + threadIdx.x;
    if (n < N) out[(size_t)b * N + n] = n < nv ? (float)(gb * (double)sf_y(Fr, n)) : 0.0f;
  }
}

extern "C" int sa_srcfilt_synth(const float* wav, const float* exc, const int* n_valid, int B, int N, int level,
                                float* out, void* ws, int* status, float* gain, void* stream) {
  if (!wav || !exc || !n_valid || !out || !ws || !sf_dims_ok(B, N)) return -EINVAL;
  const int T = sf_synth_frames(N);
  const int nblk = sa_div_up(N, SF_CHUNK);
  float* F = (float*)ws;
  double* sums = (double*)(F + (size_t)B * T * SF_W);       // 1280 bytes per frame: 8-byte aligned
  double* g = sums + 2 * (size_t)B * nblk;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sa_srcfilt_frame_kernel, dim3(T, B), dim3(SF_THREADS), 0, s, wav, exc, n_valid, N, T, F, status);
  if (level)
    hipLaunchKernelGGL(sa_srcfilt_sums_kernel, dim3(nblk, B), dim3(SF_SUM_THREADS), 0, s, wav, n_valid, N, T,
                       (const float*)F, sums);
  hipLaunchKernelGGL(sa_srcfilt_gain_kernel, dim3(B), dim3(64), 0, s, (const double*)sums, nblk, level, g, gain);
  hipLaunchKernelGGL(sa_srcfilt_apply_kernel, dim3(sa_div_up(N, SF_APPLY), B), dim3(256), 0, s, n_valid, N, T,
                     (const float*)F, (const double*)g, out);
  return -(int)hipGetLastError();
}
