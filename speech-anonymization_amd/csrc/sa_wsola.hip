// WSOLA time-scale modification (timescale.TimeScaler): 20 ms windows of the input are copied to the
// output at a fixed hop, and each window's position is chosen within +-10 ms of where the tempo says it should be, so
// that it continues the previous one.  Pitch and envelope stay by construction; the duration changes.  No STFT, no
// phase, no iteration, no random number.
//   sa_wsola_quant    wav -> the row peaks, then the search signal q (int16) of every row
//   sa_wsola_search   q, tempo_q -> the position of every window: a serial chain of argmins, one workgroup per row
//   sa_wsola_ola      the overlap-add in gather form: every output sample reads the two windows that reach it
// Every decision is made on integers (include/sa_hip.h states the algorithm); the overlap-add is two fp32 products and
// one fp32 sum, each rounded on its own.  Plain HIP C++, no atomics, fixed orders: the same bits on every run.
#include "sa_common.h"
#include <errno.h>
#include <math.h>

#pragma clang fp contract(off)

#define WS_H 160                         // hop
#define WS_W 320                         // window
#define WS_D 160                         // tolerance
#define WS_Q 16383                       // the search signal's full scale
#define WS_MAX_N (1 << 24)
#define WS_MAX_NOUT (1 << 25)
#define WS_ONE (1 << 16)
#define WS_QTILE 4096                    // samples per workgroup of the two quantisation passes
#define WS_THREADS 256
#define WS_CHUNK 8192                    // samples per staged chunk of sa_wsola_search
#define WS_BIAS 16384                    // q is staged as q + 16384, an unsigned 16-bit value
#define WS_R 8                           // candidates per lane: c, c + 2, .., c + 14 share a register window
#define WS_SEG 5                         // the 320 samples of a window are split into 5 segments ..
#define WS_SEGDW 32                      // .. of 32 packed pairs
#define WS_GROUPS 21                     // groups of 16 candidates (8 even, 8 odd): 21 * 16 = 336 >= 321
#define WS_CAND (WS_GROUPS * 2 * WS_R)   // 336
#define WS_SPAN (WS_CAND - 1 + WS_W + 1) // samples from lo on that the candidates' lanes read: up to lo + 655
#define WS_OTILE 1024                    // samples per workgroup of sa_wsola_ola: four per thread

extern "C" int sa_wsola_dim(int which) {
  switch (which) {
    case 0: return WS_H;
    case 1: return WS_W;
    case 2: return WS_D;
    case 3: return WS_Q;
    case 4: return WS_CHUNK;
    case 5: return WS_OTILE;
    case 6: return WS_QTILE;
    default: return -EINVAL;
  }
}

static inline bool ws_dims_ok(int B, int N) { return B >= 1 && B <= 65535 && N >= 1 && N <= WS_MAX_N; }
static inline int ws_parts(int N) { return (N + 3 + WS_QTILE - 1) / WS_QTILE; }
static inline long long ws_q_bytes(int B, int N) { return (2LL * B * N + 15) & ~15LL; }

extern "C" long long sa_wsola_workspace_bytes(int B, int N) {
  if (!ws_dims_ok(B, N)) return -EINVAL;
  return ws_q_bytes(B, N) + ((4LL * B * ws_parts(N) + 15) & ~15LL);
}

__host__ __device__ static inline int ws_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// n_out of a row of n valid samples before the cap: (n 2^16 + tempo_q / 2) / tempo_q, tempo_q in [2^15, 2^17]
__host__ __device__ static inline int ws_out_len(int n, int tempo_q) {
  const long long tq = ws_clamp(tempo_q, WS_ONE / 2, 2 * WS_ONE);
  return n <= 0 ? 0 : (int)((((long long)n << 16) + tq / 2) / tq);
}

extern "C" int sa_wsola_out_len(int n, int tempo_q) {
  if (n < 0 || n > WS_MAX_N) return -EINVAL;
  return ws_out_len(n, tempo_q);
}

// ---- quantisation ------------------------------------------------------------------------------------
// Both passes walk a row in groups of four samples that are 16-byte aligned in memory: group g of a row whose first
// sample is sh samples past a 16-byte boundary holds the samples 4 g - sh .. 4 g - sh + 3.  A group that lies in the row
// whole is one 16-byte load; the (at most two) others are read sample by sample.
__device__ static inline void ws_load4(const float* __restrict__ x, int i0, int N, float* v) {
  if (i0 >= 0 && i0 + 4 <= N) {
    const float4 u = *reinterpret_cast<const float4*>(x + i0);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (i0 + e >= 0 && i0 + e < N) ? x[i0 + e] : 0.0f;
  }
}

__device__ static inline float ws_block_max(float m, float* red) {
  m = sa_wave_max(m);
  if ((threadIdx.x & (SA_WAVE - 1)) == 0) red[threadIdx.x / SA_WAVE] = m;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < WS_THREADS / SA_WAVE; ++w) r = fmaxf(r, red[w]);
  return r;
}

// grid (P, B): the largest finite |wav[n]|, n < n_valid, of 4096 samples -> part[b][tile]
__global__ __launch_bounds__(WS_THREADS) void sa_wsola_peak_kernel(const float* __restrict__ wav,
                                                                   const int* __restrict__ n_valid, int N, int P,
                                                                   float* __restrict__ part) {
  __shared__ float red[WS_THREADS / SA_WAVE];
  const int b = blockIdx.y, nv = ws_clamp(n_valid[b], 0, N);
  const float* x = wav + (size_t)b * N;
  const int sh = (int)(((uintptr_t)x >> 2) & 3);
  float m = 0.0f;
#pragma unroll
  for (int j = 0; j < WS_QTILE / 4 / WS_THREADS; ++j) {
    const int i0 = 4 * (blockIdx.x * (WS_QTILE / 4) + j * WS_THREADS + threadIdx.x) - sh;
    if (i0 >= nv) continue;
    float v[4];
    ws_load4(x, i0, N, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = fabsf(v[e]);
      if (i0 + e >= 0 && i0 + e < nv && a < INFINITY) m = fmaxf(m, a);      // (a NaN fails the comparison)
    }
  }
  m = ws_block_max(m, red);
  if (threadIdx.x == 0) part[(size_t)b * P + blockIdx.x] = m;
}

// grid (P, B): the row's peak from its partial maxima, then q of 4096 samples
__global__ __launch_bounds__(WS_THREADS) void sa_wsola_q_kernel(const float* __restrict__ wav,
                                                                const int* __restrict__ n_valid, int N, int P,
                                                                const float* __restrict__ part,
                                                                short* __restrict__ qg) {
  __shared__ float red[WS_THREADS / SA_WAVE];
  const int b = blockIdx.y, nv = ws_clamp(n_valid[b], 0, N);
  const float* x = wav + (size_t)b * N;
  short* q = qg + (size_t)b * N;
  const int sh = (int)(((uintptr_t)x >> 2) & 3);
  float m = 0.0f;
  for (int i = threadIdx.x; i < P; i += WS_THREADS) m = fmaxf(m, part[(size_t)b * P + i]);
  const double s = (double)ws_block_max(m, red);
#pragma unroll
  for (int j = 0; j < WS_QTILE / 4 / WS_THREADS; ++j) {
    const int i0 = 4 * (blockIdx.x * (WS_QTILE / 4) + j * WS_THREADS + threadIdx.x) - sh;
    if (i0 >= N) continue;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i0 < nv) ws_load4(x, i0, N, v);
    short r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool live = i0 + e < nv && fabsf(v[e]) < INFINITY && s > 0.0;
      r[e] = live ? (short)(int)rint(((double)v[e] * (double)WS_Q) / s) : (short)0;
    }
    if (i0 >= 0 && i0 + 4 <= N && (((uintptr_t)(q + i0)) & 7) == 0) {
      *reinterpret_cast<short4*>(q + i0) = make_short4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e >= 0 && i0 + e < N) q[i0 + e] = r[e];
    }
  }
}

static int ws_quant_launch(const float* wav, const int* n_valid, int B, int N, void* ws, hipStream_t st) {
  const int P = ws_parts(N);
  float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + ws_q_bytes(B, N));
  hipLaunchKernelGGL(sa_wsola_peak_kernel, dim3(P, B), dim3(WS_THREADS), 0, st, wav, n_valid, N, P, part);
  hipLaunchKernelGGL(sa_wsola_q_kernel, dim3(P, B), dim3(WS_THREADS), 0, st, wav, n_valid, N, P, part,
                     static_cast<short*>(ws));
  return -(int)hipGetLastError();
}

extern "C" int sa_wsola_quant(const float* wav, const int* n_valid, int B, int N, void* ws, void* stream) {
  if (!wav || !n_valid || !ws || !ws_dims_ok(B, N)) return -EINVAL;
  return ws_quant_launch(wav, n_valid, B, N, ws, (hipStream_t)stream);
}

// ---- search ------------------------------------------------------------------------------------------
// The staged chunk: sa[i] = q[c0 + i] + 16384 for i < 8192 + 8 (16384, q = 0, outside the row's valid samples), and
// sb[i] = sa[i + 1], so that a window that starts at an odd distance from c0 is read as aligned pairs too.
__device__ static inline unsigned ws_pair(const unsigned* sa, const unsigned* sb, int e, int j) {
  return ((e & 1) ? sb : sa)[(e >> 1) + j];
}

__device__ static inline unsigned long long ws_min_u64(unsigned long long a, unsigned long long b) {
  return a < b ? a : b;
}

// grid (B), one workgroup of 256 per row.  A step: lanes 0..209 are (group of 16 candidates, parity, segment); a lane
// holds 39 packed pairs of the candidates' span in registers and slides eight candidates c, c + 2, .., c + 14 over them
// against 32 pairs of the template, 256 packed sums of absolute differences; the segment sums meet in LDS, every
// candidate's key (cost, |c - a|, c) is formed, and the least key is reduced through the waves.  Nothing on the chain
// reads global memory but the re-staging: a step's reads span at most 823 samples and the windows advance by
// 160 tempo <= 320 a step, so a chunk serves 23 steps at the least.
__global__ __launch_bounds__(WS_THREADS) void sa_wsola_search_kernel(const short* __restrict__ qg,
                                                                     const int* __restrict__ tempo_q,
                                                                     const int* __restrict__ n_valid, int N, int Nout,
                                                                     int Kcap,
                                                                     int* __restrict__ pos, int* __restrict__ count,
                                                                     int* __restrict__ n_out) {
  __shared__ __attribute__((aligned(16))) unsigned sa[(WS_CHUNK + 8) / 2];
  __shared__ __attribute__((aligned(16))) unsigned sb[WS_CHUNK / 2];
  __shared__ unsigned part[WS_SEG][WS_CAND];
  __shared__ unsigned long long wmin[2][WS_THREADS / SA_WAVE];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int nv = ws_clamp(n_valid[b], 0, N);
  const long long tq = ws_clamp(tempo_q[b], WS_ONE / 2, 2 * WS_ONE);
  const int no = min(Nout, ws_out_len(nv, (int)tq));
  const int K = no > 0 ? min((no - 1) / WS_H + 1, Kcap) : 0;
  const long long row = (long long)b * N;
  const short* q = qg + row;
  int* pk = pos + (size_t)b * Kcap;
  if (tid == 0) {
    count[b] = K;
    n_out[b] = no;
    if (K > 0) pk[0] = 0;
  }
  // this lane's share of a step
  const int seg = tid / (2 * WS_GROUPS), gp = tid - seg * (2 * WS_GROUPS);      // gp = 2 group + parity
  const int coff = (gp >> 1) * (2 * WS_R) + (gp & 1);                          // its first candidate, from lo on
  const bool worker = tid < WS_SEG * 2 * WS_GROUPS;

  long long c0 = 0;
  bool staged = false;
  int p = 0;
  for (int k = 1; k < K; ++k) {
    const int a = (int)(((long long)k * WS_H * tq + (WS_ONE / 2)) >> 16);
    const int t = p + WS_H;
    const int lo = max(a - WS_D, 0), hi = min(a + WS_D, max(nv - 1, 0));
    if (hi <= lo) {                                           // (the same in every thread) one candidate
      p = hi;
      if (tid == 0) pk[k] = p;
      continue;
    }
    const int first = min(t, lo), last = max(t + WS_W, lo + WS_SPAN);
    if (!staged || first < c0 || last > c0 + WS_CHUNK) {
      __syncthreads();
      c0 = ((row + first) & ~7LL) - row;                      // 16-byte aligned in the workspace; first - 7 at the least
      for (int i = tid; i < (WS_CHUNK + 8) / 8; i += WS_THREADS) {
        const long long s0 = c0 + 8LL * i;
        unsigned short v[8];
        if (s0 + 8 <= (long long)nv && s0 >= 0) {
          const uint4 u = *reinterpret_cast<const uint4*>(q + s0);
          const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[2 * e] = (unsigned short)(w[e] & 0xffffu);
            v[2 * e + 1] = (unsigned short)(w[e] >> 16);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const long long s = s0 + e;
            v[e] = (s >= 0 && s < (long long)nv) ? (unsigned short)q[s] : (unsigned short)0;
          }
        }
        uint4 o;
        unsigned* od = reinterpret_cast<unsigned*>(&o);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          od[e] = ((unsigned)(unsigned short)(v[2 * e] + WS_BIAS)) |
                  ((unsigned)(unsigned short)(v[2 * e + 1] + WS_BIAS) << 16);
        *reinterpret_cast<uint4*>(&sa[4 * i]) = o;
      }
      __syncthreads();
      for (int j = tid; j < WS_CHUNK / 2; j += WS_THREADS) sb[j] = (sa[j] >> 16) | (sa[j + 1] << 16);
      staged = true;
      __syncthreads();
    }
    if (worker) {
      const int ec = (int)(lo + coff - c0) + 2 * WS_SEGDW * seg;
      const int et = (int)(t - c0) + 2 * WS_SEGDW * seg;
      unsigned cd[WS_SEGDW + WS_R - 1];
#pragma unroll
      for (int j = 0; j < WS_SEGDW + WS_R - 1; ++j) cd[j] = ws_pair(sa, sb, ec, j);
      unsigned acc[WS_R];
#pragma unroll
      for (int r = 0; r < WS_R; ++r) acc[r] = 0u;
#pragma unroll
      for (int j = 0; j < WS_SEGDW; ++j) {
        const unsigned tj = ws_pair(sa, sb, et, j);
#pragma unroll
        for (int r = 0; r < WS_R; ++r) acc[r] = __builtin_amdgcn_sad_u16(tj, cd[j + r], acc[r]);
      }
#pragma unroll
      for (int r = 0; r < WS_R; ++r) part[seg][coff + 2 * r] = acc[r];
    }
    __syncthreads();
    unsigned long long key = ~0ull;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = tid + h * WS_THREADS;
      if (i <= hi - lo) {
        unsigned cost = 0u;
#pragma unroll
        for (int s = 0; s < WS_SEG; ++s) cost += part[s][i];
        const int c = lo + i;
        key = ws_min_u64(key, ((unsigned long long)cost << 34) | ((unsigned long long)(unsigned)abs(c - a) << 25) |
                                  (unsigned long long)(unsigned)c);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = ws_min_u64(key, __shfl_xor(key, o, 64));
    if ((tid & (SA_WAVE - 1)) == 0) wmin[k & 1][tid / SA_WAVE] = key;
    __syncthreads();
    key = ws_min_u64(ws_min_u64(wmin[k & 1][0], wmin[k & 1][1]), ws_min_u64(wmin[k & 1][2], wmin[k & 1][3]));
    p = (int)(key & 0x1ffffffull);
    if (tid == 0) pk[k] = p;
  }
}

static int ws_search_launch(const void* ws, const int* tempo_q, const int* n_valid, int B, int N, int Nout, int* pos,
                            int* count, int* n_out, hipStream_t st) {
  hipLaunchKernelGGL(sa_wsola_search_kernel, dim3(B), dim3(WS_THREADS), 0, st, static_cast<const short*>(ws), tempo_q,
                     n_valid, N, Nout, (Nout - 1) / WS_H + 1, pos, count, n_out);
  return -(int)hipGetLastError();
}

static inline bool ws_out_ok(int Nout) { return Nout >= 1 && Nout <= WS_MAX_NOUT; }

extern "C" int sa_wsola_search(const void* ws, const int* tempo_q, const int* n_valid, int B, int N, int Nout,
                               int* pos, int* count, int* n_out, void* stream) {
  if (!ws || !tempo_q || !n_valid || !pos || !count || !n_out || !ws_dims_ok(B, N) || !ws_out_ok(Nout))
    return -EINVAL;
  return ws_search_launch(ws, tempo_q, n_valid, B, N, Nout, pos, count, n_out, (hipStream_t)stream);
}

// ---- overlap-add -------------------------------------------------------------------------------------
__device__ static inline float ws_x(const float* __restrict__ x, int i, int nv) { return i < nv ? x[i] : 0.0f; }

// grid (tiles of 1024 samples, B); a thread forms four consecutive output samples, which lie in one frame (4 divides
// 160), and stores them as 16 bytes where the address allows.  A NaN of the sum is written as 0x7fc00000.
__global__ __launch_bounds__(WS_THREADS) void sa_wsola_ola_kernel(const float* __restrict__ wav,
                                                                  const int* __restrict__ pos,
                                                                  const int* __restrict__ count,
                                                                  const int* __restrict__ tempo_q,
                                                                  const int* __restrict__ n_valid,
                                                                  const float* __restrict__ hann, int N, int Nout,
                                                                  int Kcap, float* __restrict__ out) {
  const int b = blockIdx.y, m0 = blockIdx.x * WS_OTILE + 4 * threadIdx.x;
  if (m0 >= Nout) return;
  const int nv = ws_clamp(n_valid[b], 0, N);
  const int no = min(Nout, ws_out_len(nv, tempo_q[b]));
  const int K = ws_clamp(count[b], 0, Kcap);
  const float* x = wav + (size_t)b * N;
  float* y = out + (size_t)b * Nout + m0;
  const int k = m0 / WS_H, r0 = m0 - k * WS_H;
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (m0 < no && k < K) {
    const int* pk = pos + (size_t)b * Kcap;
    const int p1 = ws_clamp(pk[k], 0, N);
    const int p0 = k > 0 ? ws_clamp(pk[k - 1], 0, N) + WS_H : p1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = r0 + e;
      if (m0 + e >= no) continue;
      const float x1 = ws_x(x, p1 + r, nv);
      if (p0 == p1) {
        v[e] = x1;
      } else {
        const float a = hann[r] * x1, c = hann[r + WS_H] * ws_x(x, p0 + r, nv);     // (contraction is off in this file)
        const float s = a + c;
        v[e] = s != s ? __uint_as_float(0x7fc00000u) : s;
      }
    }
  }
  if (m0 + 4 <= Nout && (((uintptr_t)y) & 15) == 0) {
    *reinterpret_cast<float4*>(y) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (m0 + e < Nout) y[e] = v[e];
  }
}

static int ws_ola_launch(const float* wav, const int* pos, const int* count, const int* tempo_q, const int* n_valid,
                         const float* hann, int B, int N, int Nout, float* out, hipStream_t st) {
  hipLaunchKernelGGL(sa_wsola_ola_kernel, dim3(sa_div_up(Nout, WS_OTILE), B), dim3(WS_THREADS), 0, st, wav, pos, count,
                     tempo_q, n_valid, hann, N, Nout, (Nout - 1) / WS_H + 1, out);
  return -(int)hipGetLastError();
}

static inline bool ws_alias(const float* wav, const float* out, int B, int N, int Nout) {
  const uintptr_t a0 = (uintptr_t)wav, a1 = a0 + 4ull * B * N, b0 = (uintptr_t)out, b1 = b0 + 4ull * B * Nout;
  return a0 < b1 && b0 < a1;
}

extern "C" int sa_wsola_ola(const float* wav, const int* pos, const int* count, const int* tempo_q,
                            const int* n_valid, const float* hann, int B, int N, int Nout, float* out, void* stream) {
  if (!wav || !pos || !count || !tempo_q || !n_valid || !hann || !out || !ws_dims_ok(B, N) || !ws_out_ok(Nout) ||
      ws_alias(wav, out, B, N, Nout))
    return -EINVAL;
  return ws_ola_launch(wav, pos, count, tempo_q, n_valid, hann, B, N, Nout, out, (hipStream_t)stream);
}

extern "C" int sa_wsola(const float* wav, const int* tempo_q, const int* n_valid, const float* hann, int B, int N,
                        int Nout, void* ws, float* out, int* pos, int* count, int* n_out, void* stream) {
  if (!wav || !tempo_q || !n_valid || !hann || !ws || !out || !pos || !count || !n_out || !ws_dims_ok(B, N) ||
      !ws_out_ok(Nout) || ws_alias(wav, out, B, N, Nout))
    return -EINVAL;
  hipStream_t st = (hipStream_t)stream;
  int rc = ws_quant_launch(wav, n_valid, B, N, ws, st);
  if (rc) return rc;
  rc = ws_search_launch(ws, tempo_q, n_valid, B, N, Nout, pos, count, n_out, st);
  if (rc) return rc;
  return ws_ola_launch(wav, pos, count, tempo_q, n_valid, hann, B, N, Nout, out, st);
}
