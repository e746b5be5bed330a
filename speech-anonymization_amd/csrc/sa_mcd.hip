// Mel-cepstral distortion along a banded DTW alignment (ops.mcd): mel_ref [B][T_ref][n_mels],
// mel_deg [B][T_deg][n_mels] fp32 log-Mel power in dB, n_ref, n_deg [B] -> mcd, mcd_sync [B] fp32, frames [B] int32.
// Every step in fp64 (include/sa_hip.h carries the definition).  Three launches, only the last one serial:
//   cepstra     c_k(t), k = 1..K, of the frames below a row's count, both inputs in one grid.  A workgroup builds the
//               cosine table cos(pi k (2m + 1) / (2 n_mels)) in LDS once (the angle reduced as an integer mod
//               4 n_mels, so cospi sees an argument in [0, 2)) and takes 32 frames, 8 at a time, a thread per
//               (frame, k), the sum over m in order.
//   band        d(i, j) of every cell of the band, a thread per cell, the sum over k in order, stored by
//               anti-diagonal: D[b][s][p] holds the cell i + j = s, j - i = o with o = omin(s) + 2 p, where
//               omin(s) = -R + ((R + s) & 1) is the smallest offset in [-R, R] of the parity of s; p = 0..R.  A
//               place that is no cell (i or j outside the row's counts, o > R) holds 0 and is never read into a
//               result.
//   recurrence  one wave per row, lane p the cell p of the anti-diagonal.  The predecessors of a cell sit at the same
//               lane two anti-diagonals back (i-1, j-1), and on the previous one at the lanes p + a (i-1, j) and
//               p + a - 1 (i, j-1) with a = (R + s) & 1: one whole-wave DPP shift up or down per step, no LDS, no
//               barrier.
//               The loads of D do not depend on the recurrence: the wave reads MC_AHEAD anti-diagonals (coalesced,
//               8 (R + 1) bytes each) while it walks the MC_AHEAD before them.  The lane of offset 0 adds d(i, i)
//               in the order of i for the frame-synchronous figure.
// One path for every T.  No atomics, every sum in a fixed order: the same bits on every run.
#include "sa_common.h"
#include <errno.h>

#define MC_MAX_BAND 63
#define MC_MAX_ORDER 32
#define MC_MAX_MELS 128
#define MC_MAX_T 104858                   // the frames of 2^24 samples
#define MC_MAX_B 65535                    // grid.y
#define MC_CEP_FRAMES 32                  // frames per workgroup of the cepstra kernel, 8 x 32 threads at a time
#define MC_BAND_THREADS 256
#define MC_AHEAD 16                       // anti-diagonals in flight in the recurrence

extern "C" int sa_mcd_dim(int which) {
  switch (which) {
    case 0: return MC_MAX_BAND;
    case 1: return MC_MAX_ORDER;
    case 2: return MC_MAX_MELS;
    case 3: return MC_MAX_T;
    default: return -EINVAL;
  }
}

__device__ static inline int mc_count(const int* __restrict__ n, int b, int T) { return min(max(n[b], 0), T); }

// grid (ceil(max(T_ref, T_deg) / 32), B, 2): z = 0 ref, 1 deg
__global__ __launch_bounds__(256) void sa_mcd_cepstra_kernel(const float* __restrict__ mel_ref,
                                                             const float* __restrict__ mel_deg,
                                                             const int* __restrict__ n_ref,
                                                             const int* __restrict__ n_deg, int T_ref, int T_deg,
                                                             int n_mels, int K, double* __restrict__ cep_ref,
                                                             double* __restrict__ cep_deg) {
  __shared__ double tab[MC_MAX_MELS * MC_MAX_ORDER];        // [m][k - 1], 32 KB; the columns k <= K are filled
  const int b = blockIdx.y, which = blockIdx.z;
  const int T = which ? T_deg : T_ref;
  const int n = mc_count(which ? n_deg : n_ref, b, T);
  const int t0 = blockIdx.x * MC_CEP_FRAMES;
  if (t0 >= n) return;                                      // (uniform per workgroup: before the barrier)
  for (int e = threadIdx.x; e < n_mels * K; e += 256) {
    const int m = e / K, k = e % K + 1;
    const int q = (k * (2 * m + 1)) % (4 * n_mels);         // pi q / (2 n_mels), q in [0, 4 n_mels)
    tab[m * MC_MAX_ORDER + k - 1] = cospi((double)q / (double)(2 * n_mels));
  }
  __syncthreads();
  const int k = threadIdx.x & 31;
  if (k >= K) return;
  const float* src = (which ? mel_deg : mel_ref) + (size_t)b * T * n_mels;
  double* dst = (which ? cep_deg : cep_ref) + (size_t)b * T * K;
  for (int t = t0 + (threadIdx.x >> 5); t < min(t0 + MC_CEP_FRAMES, n); t += 8) {
    const float* x = src + (size_t)t * n_mels;
    double acc = 0.0;
    for (int m = 0; m < n_mels; ++m) acc = fma((double)x[m], tab[m * MC_MAX_ORDER + k], acc);
    dst[(size_t)t * K + k] = acc / (double)n_mels;
  }
}

// the smallest offset in [-R, R] of the parity of the anti-diagonal s
__device__ static inline int mc_omin(int s, int R) { return -R + ((R + s) & 1); }

// grid (ceil((T_ref + T_deg - 1) (R + 1) / 256), B)
__global__ __launch_bounds__(MC_BAND_THREADS) void sa_mcd_band_kernel(const double* __restrict__ cep_ref,
                                                                      const double* __restrict__ cep_deg,
                                                                      const int* __restrict__ n_ref,
                                                                      const int* __restrict__ n_deg, int T_ref,
                                                                      int T_deg, int K, int R,
                                                                      double* __restrict__ D) {
  const int b = blockIdx.y, W = R + 1;
  const long long S = (long long)T_ref + T_deg - 1;
  const long long e = (long long)blockIdx.x * MC_BAND_THREADS + threadIdx.x;
  if (e >= S * W) return;
  const int s = (int)(e / W), p = (int)(e % W);
  const int N = mc_count(n_ref, b, T_ref), M = mc_count(n_deg, b, T_deg);
  const int o = mc_omin(s, R) + 2 * p;
  const int i = (s - o) >> 1, j = (s + o) >> 1;             // (s - o even; a negative value stays negative)
  double d = 0.0;
  if (o <= R && i >= 0 && i < N && j >= 0 && j < M) {
    const double* x = cep_ref + ((size_t)b * T_ref + i) * K;
    const double* y = cep_deg + ((size_t)b * T_deg + j) * K;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const double df = x[k] - y[k];
      acc = fma(df, df, acc);
    }
    d = sqrt(0.5 * acc);
  }
  D[(size_t)b * S * W + e] = d;
}

// g of the lane below (p - 1) or above (p + 1), `edge` where there is none: a whole-wave DPP shift of each half
__device__ static inline double mc_from_below(double v, double edge) {
  const long long a = __double_as_longlong(v), e = __double_as_longlong(edge);
  const int lo = __builtin_amdgcn_update_dpp((int)e, (int)a, 0x138, 0xf, 0xf, false);                // wave_shr:1
  const int hi = __builtin_amdgcn_update_dpp((int)(e >> 32), (int)(a >> 32), 0x138, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ static inline double mc_from_above(double v, double edge) {
  const long long a = __double_as_longlong(v), e = __double_as_longlong(edge);
  const int lo = __builtin_amdgcn_update_dpp((int)e, (int)a, 0x130, 0xf, 0xf, false);                // wave_shl:1
  const int hi = __builtin_amdgcn_update_dpp((int)(e >> 32), (int)(a >> 32), 0x130, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// One anti-diagonal s with a = (R + s) & 1 = A: (i-1, j) sits at the lane p + A and (i, j-1) at the lane p + A - 1 of
// the previous anti-diagonal, i.e. this lane and the one above (A = 1) or below (A = 0).  lo, hi: the s at which this
// lane is a cell for either a; diag: this lane holds d(i, i) on this anti-diagonal.
template <int A>
__device__ static inline void mc_step(int s, double d, const int* lo, const int* hi, bool diag, int L, double& g1,
                                      double& g2, double& sync) {
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const double gn = A ? mc_from_above(g1, inf) : mc_from_below(g1, inf);
  const double g = fmin(g2 + 2.0 * d, fmin(g1, gn) + d);
  if (diag && (s >> 1) < L) sync += d;                      // i = s / 2
  g2 = g1;
  g1 = s >= lo[A] && s < hi[A] ? g : inf;
}

// grid B, one wave; PAR = R & 1, so that a is known where the steps are unrolled (MC_AHEAD is even)
template <int PAR>
__global__ __launch_bounds__(64) void sa_mcd_dtw_kernel(const double* __restrict__ D, const int* __restrict__ n_ref,
                                                        const int* __restrict__ n_deg, int T_ref, int T_deg, int R,
                                                        float* __restrict__ mcd, float* __restrict__ mcd_sync,
                                                        int* __restrict__ frames) {
  const int b = blockIdx.x, p = threadIdx.x, W = R + 1;
  const int N = mc_count(n_ref, b, T_ref), M = mc_count(n_deg, b, T_deg);
  if (N < 1 || M < 1 || abs(N - M) > R) {                   // (uniform)
    if (p == 0) mcd[b] = 0.0f, mcd_sync[b] = 0.0f, frames[b] = 0;
    return;
  }
  const size_t Sfull = (size_t)T_ref + T_deg - 1;
  const double* Db = D + (size_t)b * Sfull * W;
  const int S = N + M - 1, L = min(N, M);
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const bool has = p < W;                                   // the lanes that have a place in D
  const int p0 = (R - PAR) >> 1;                            // the lane of offset 0 on an even anti-diagonal
  const bool mid = p == p0;
  // this lane's offset on the anti-diagonals with a = 0 and a = 1, and the s at which it is a cell there:
  // 0 <= i = (s - o) / 2 < N and 0 <= j = (s + o) / 2 < M, i.e. |o| <= s < min(2 N + o, 2 M - o); none when o > R
  int lo[2], hi[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int o = -R + a + 2 * p;
    lo[a] = abs(o);
    hi[a] = o <= R ? min(2 * N + o, 2 * M - o) : 0;
  }
  // the anti-diagonals s - 1 and s - 2 at this lane; g(0, 0) = 2 d(0, 0) comes out of the step from a 0 at (-1, -1)
  double g1 = inf, g2 = mid ? 0.0 : inf, sync = 0.0;
  double cur[MC_AHEAD], nxt[MC_AHEAD];
#pragma unroll
  for (int u = 0; u < MC_AHEAD; ++u) cur[u] = has && u < S ? Db[(size_t)u * W + p] : 0.0;
  int s0 = 0;
  for (; s0 + MC_AHEAD <= S; s0 += MC_AHEAD) {              // whole groups of MC_AHEAD anti-diagonals: no test per step
#pragma unroll
    for (int u = 0; u < MC_AHEAD; ++u) {
      const int s = s0 + MC_AHEAD + u;
      nxt[u] = has && s < S ? Db[(size_t)s * W + p] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < MC_AHEAD; u += 2) {                 // (s0 and u are even: a = PAR, then PAR ^ 1)
      mc_step<PAR>(s0 + u, cur[u], lo, hi, mid, L, g1, g2, sync);
      mc_step<PAR ^ 1>(s0 + u + 1, cur[u + 1], lo, hi, false, L, g1, g2, sync);
    }
#pragma unroll
    for (int u = 0; u < MC_AHEAD; ++u) cur[u] = nxt[u];
  }
#pragma unroll
  for (int u = 0; u < MC_AHEAD; u += 2) {                   // the last S - s0 < MC_AHEAD anti-diagonals (uniform tests)
    if (s0 + u < S) mc_step<PAR>(s0 + u, cur[u], lo, hi, mid, L, g1, g2, sync);
    if (s0 + u + 1 < S) mc_step<PAR ^ 1>(s0 + u + 1, cur[u + 1], lo, hi, false, L, g1, g2, sync);
  }
  // g(N-1, M-1): the anti-diagonal S - 1, offset M - N
  const int last = ((M - N) - mc_omin(S - 1, R)) >> 1;
  if (p == last) mcd[b] = (float)(g1 / (double)(N + M)), frames[b] = N + M;
  if (mid) mcd_sync[b] = (float)(sync / (double)L);
}

extern "C" int sa_mcd(const float* mel_ref, const float* mel_deg, const int* n_ref, const int* n_deg, int B, int T_ref,
                      int T_deg, int n_mels, int order, int band, void* ws, float* mcd, float* mcd_sync, int* frames,
                      void* stream) {
  if (!mel_ref || !mel_deg || !n_ref || !n_deg || !ws || !mcd || !mcd_sync || !frames || B < 1 || B > MC_MAX_B ||
      T_ref < 1 || T_ref > MC_MAX_T || T_deg < 1 || T_deg > MC_MAX_T || n_mels < 2 || n_mels > MC_MAX_MELS ||
      order < 1 || order > MC_MAX_ORDER || order >= n_mels || band < 0 || band > MC_MAX_BAND)
    return -EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double* cep_ref = (double*)ws;
  double* cep_deg = cep_ref + (size_t)B * T_ref * order;
  double* D = cep_deg + (size_t)B * T_deg * order;
  const int Tm = T_ref > T_deg ? T_ref : T_deg;
  hipLaunchKernelGGL(sa_mcd_cepstra_kernel, dim3(sa_div_up(Tm, MC_CEP_FRAMES), B, 2), dim3(256), 0, st, mel_ref,
                     mel_deg, n_ref, n_deg, T_ref, T_deg, n_mels, order, cep_ref, cep_deg);
  const long long cells = ((long long)T_ref + T_deg - 1) * (band + 1);
  hipLaunchKernelGGL(sa_mcd_band_kernel, dim3((unsigned)((cells + MC_BAND_THREADS - 1) / MC_BAND_THREADS), B),
                     dim3(MC_BAND_THREADS), 0, st, cep_ref, cep_deg, n_ref, n_deg, T_ref, T_deg, order, band, D);
  hipLaunchKernelGGL((band & 1) ? sa_mcd_dtw_kernel<1> : sa_mcd_dtw_kernel<0>, dim3(B), dim3(64), 0, st, D, n_ref,
                     n_deg, T_ref, T_deg, band, mcd, mcd_sync, frames);
  return -(int)hipGetLastError();
}
