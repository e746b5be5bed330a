// LPC source-filter resynthesis (sourcefilter.py; ops.srcfilt_pulses, ops.srcfilt_excite, ops.srcfilt_synth; DESIGN
// section 27; include/sa_hip.h carries the definition).  The classic LPC vocoder: every frame keeps its all-pole
// envelope and its energy, the residual is thrown away, and the filter is driven by a synthetic excitation -- pulses at
// the F0 track where the frame is voiced, noise elsewhere.  The pulses are laid down at whatever period is asked for, so
// the same pass moves the pitch.
//   sa_srcfilt_pulses   f0, rho_q -> where every pulse goes (pos_q, int64 in units of 2^-16 samples) and its period
//   sa_srcfilt_excite   the pulse table -> the excitation: hashed uniform noise plus the linearly interpolated pulses
//   sa_srcfilt_synth    the framing, fit, overlap-add and level matching of sa_lpc_shared.h (section 17); the frame is
//                       the all-pole filter 1 / a driven by the windowed excitation, scaled to its prediction error
// Every decision of the first two is made on integers, or on fp64 formed from the fp32 inputs; the excitation's fp32
// operations are rounded one by one.  Only the filtered output has a rounding bar.  No root finder, no FIR.
// Plain HIP C++, no atomics, fixed summation orders: the same bits on every run, and a row alone gives the bits it
// gives inside a batch.
#include "sa_lpc_shared.h"
#include <limits.h>
#include <math.h>

#define SF_H SA_FR_H
#define SF_THREADS SA_FR_THREADS
#define SF_MAX_N (1 << 24)
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
    case 0: return SA_FR_W;
    case 1: return SF_H;
    case 2: return SA_FR_P;
    case 3: return SF_THREADS;
    case 4: return SA_FR_CHUNK;
    case 5: return SF_TMIN;
    case 6: return SF_TMAX;
    case 7: return SF_KDIV;
    case 8: return SF_TILE;
    case 9: return SF_G;
    default: return -EINVAL;
  }
}

static inline bool sf_dims_ok(int B, int N) { return B >= 1 && B <= SA_FR_MAX_B && N >= 1 && N <= SF_MAX_N; }
static inline bool sf_frames_ok(int N, int T) { return T == N / SF_H + 1 || T == (N + SF_H - 1) / SF_H + 1; }

extern "C" long long sa_srcfilt_workspace_bytes(int B, int N) {
  if (!sf_dims_ok(B, N)) return -EINVAL;
  return 4LL * B * sa_fr_frames(N) * SA_FR_W + 8LL * (2LL * B * sa_div_up(N, SA_FR_CHUNK) + B);
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
// grid (T, B), one wave; sa_fr_roots_kernel's framing, fit, recursion and store (sa_lpc_shared.h) without its roots
// and its FIR.  LDS: the windowed frame with 20 zeros on either side (the lag sums' far end reads zeros instead of
// branching), the windowed excitation, the output.
//   (a) lane j mod 64 windows five samples of the frame and of the excitation
//   (b) lane (k, part) sums lag k over a third of the frame; the three parts are added in order: sa_mcadams's sums
//   (c) every lane runs the Levinson recursion on the same values, unrolled in registers
//   (d) Ee: five squares per lane in order, the wave by butterfly
//   (e) IIR: the 320-step recursion on g ex, the same in every lane, its history a register ring
__global__ __launch_bounds__(SA_FR_THREADS) void sa_srcfilt_frame_kernel(const float* __restrict__ wav,
                                                                         const float* __restrict__ exc,
                                                                         const int* __restrict__ n_valid, int N, int T,
                                                                         float* __restrict__ ws,
                                                                         int* __restrict__ status) {
  __shared__ double fs[SA_FR_P + SA_FR_W + SA_FR_P];
  __shared__ double es[SA_FR_W];
  __shared__ double ys[SA_FR_W];
  __shared__ double part[SA_FR_THREADS];
  const int lane = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
  double wv[5], a[SA_FR_P + 1], ee = 0.0, err = 0.0;
  // (a), (b), (c)
  sa_fr_load<true>(wav, exc, b, t, N, sa_fr_valid(n_valid, b, N), lane, fs, es, wv, ee);
  int st = sa_lpc_fit<SA_FR_P, SA_FR_W, SA_FR_PART, SA_FR_P>(fs, part, lane, a, err);
  // (d)
  ee = sa_wave_sum_d(ee);
  if (st == 0 && ee < SF_NO_EXC) st = 3;

  if (st == 0) {
    // (e)
    const double g = sqrt(err / ee);
    sa_fr_allpole(a, [&](int j) { return g * es[j]; }, ys);
  }
  __syncthreads();
  sa_fr_store(ws + ((size_t)b * T + t) * SA_FR_W, lane, st, ys, fs, wv);
  if (status && lane == 0) status[(size_t)b * T + t] = st;
}

struct SaNoCopy {                                           // every row is synthesised: no parameter is read
  static constexpr bool COPIES = false;
};

extern "C" int sa_srcfilt_synth(const float* wav, const float* exc, const int* n_valid, int B, int N, int level,
                                float* out, void* ws, int* status, float* gain, void* stream) {
  if (!wav || !exc || !n_valid || !out || !ws || !sf_dims_ok(B, N)) return -EINVAL;
  hipLaunchKernelGGL(sa_srcfilt_frame_kernel, dim3(sa_fr_frames(N), B), dim3(SA_FR_THREADS), 0, (hipStream_t)stream,
                     wav, exc, n_valid, N, sa_fr_frames(N), (float*)ws, status);
  return sa_fr_level<SaNoCopy>(wav, nullptr, n_valid, B, N, level, out, ws, gain, (hipStream_t)stream);
}
