// STOI / ESTOI intelligibility scoring (ops.stoi): ref, deg [B][N] fp32 at 16 kHz, n_valid [B] ->
// stoi, estoi [B] fp32, frames, segments [B] int32.  Every step in fp64 (include/sa_hip.h carries the definition):
//   resample   x10[m] = sum_n x[n] h[8 m - 5 n], |8 m - 5 n| <= 80, ascending n (a gather; the taps from the host)
//   energy     e_t = sum_j (w[j] x10[128 t + j])^2 of ref, a wave per frame
//   select     max_t e_t, kept: e_t > 1e-4 max, the kept frames' indices t_0 < t_1 < ... by a ballot scan, K
//   bands      frame m of the compacted signal formed in LDS from the kept frames t_{m-1}, t_m, t_{m+1}, windowed,
//              the bins 7..218 of its 512-point DFT as a direct sum against a twiddle table, 15 band magnitudes
//   segments   per 30-frame segment the 15 STOI correlations and the ESTOI d_m, 16 lanes a segment
//   final      the partials added in a fixed order, a wave per row
// No atomics, every sum in a fixed order: the same bits on every run.
#include "sa_common.h"
#include <errno.h>

#define ST_SR10 10000
#define ST_W 256
#define ST_H 128
#define ST_NFFT 512
#define ST_NB 15
#define ST_SEG 30
#define ST_HALF 80
#define ST_TAPS (2 * ST_HALF + 1)
#define ST_FT 8                           // compacted frames per workgroup of the bands kernel (x 2 signals)
#define ST_SG 16                          // segments per workgroup: 16 lanes each
#define ST_THREADS 256
#define ST_K0 7                           // the first bin any band needs
#define ST_NK 212                         // bins 7..218
#define ST_MAX_B 65535                    // grid.y
#define ST_MAX_N (1 << 24)
#define ST_RANGE 1e-4
#define ST_CLIP (1.0 + 5.623413251903491) // 1 + 10^0.75
#define ST_EPS 2.220446049250313e-16      // 2^-52

extern "C" int sa_stoi_dim(int which) {
  switch (which) {
    case 0: return ST_SR10;
    case 1: return ST_W;
    case 2: return ST_H;
    case 3: return ST_NFFT;
    case 4: return ST_NB;
    case 5: return ST_SEG;
    case 6: return ST_TAPS;
    case 7: return ST_FT;
    case 8: return ST_SG;
    case 9: return ST_THREADS;
    default: return -EINVAL;
  }
}

__device__ static const int st_lo[ST_NB + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

__device__ static inline double st_window(int j) { return 0.5 - 0.5 * cospi((double)(2 * (j + 1)) * (1.0 / 257.0)); }
__device__ static inline int st_nvalid(const int* n_valid, int b, int N) { return min(max(n_valid[b], 0), N); }
__device__ static inline int st_n10(int nv) { return (int)((5ll * nv + 7) / 8); }
__device__ static inline int st_frames(int n10) { return n10 >= ST_W ? (n10 - ST_W) / ST_H + 1 : 0; }

// the workspace: x10 [B][2][M], e [B][F], X [B][2][15][F], part [B][F][2] (fp64), then idx [B][F], K [B] (int32)
struct StWs {
  double *x10, *e, *X, *part;
  int *idx, *K;
  int M, F;
};

// grid (blocks of 256 outputs, B, 2 signals)
__global__ __launch_bounds__(ST_THREADS) void sa_stoi_resample_kernel(const float* __restrict__ ref,
                                                                       const float* __restrict__ deg,
                                                                       const int* __restrict__ n_valid, int N,
                                                                       const double* __restrict__ taps, StWs ws) {
  __shared__ double hs[ST_TAPS];
  const int tid = threadIdx.x, b = blockIdx.y, sig = blockIdx.z;
  if (tid < ST_TAPS) hs[tid] = taps[tid];
  __syncthreads();
  const int nv = st_nvalid(n_valid, b, N), n10 = st_n10(nv);
  const int m = blockIdx.x * ST_THREADS + tid;
  if (m >= n10) return;
  const float* x = (sig ? deg : ref) + (size_t)b * N;
  const int a = 8 * m - ST_HALF;
  const int n_lo = a >= 0 ? (a + 4) / 5 : -((-a) / 5);      // ceil(a / 5)
  double acc = 0.0;
  for (int i = 0; i <= 2 * ST_HALF / 5; ++i) {
    const int n = n_lo + i, k = 8 * m - 5 * n;
    if (k < -ST_HALF) break;
    if (n >= 0 && n < nv) acc = fma((double)x[n], hs[k + ST_HALF], acc);
  }
  ws.x10[((size_t)b * 2 + sig) * ws.M + m] = acc;
}

// grid (blocks of 4 frames, B): a wave per frame of ref, lane l the samples l, l + 64, l + 128, l + 192 in order,
// the wave by butterfly
__global__ __launch_bounds__(ST_THREADS) void sa_stoi_energy_kernel(const int* __restrict__ n_valid, int N, StWs ws) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int t = blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);
  if (t >= st_frames(st_n10(st_nvalid(n_valid, b, N)))) return;
  const double* x = ws.x10 + (size_t)b * 2 * ws.M + (size_t)ST_H * t;
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < ST_W / 64; ++i) {
    const int j = lane + 64 * i;
    const double v = st_window(j) * x[j];
    acc = fma(v, v, acc);
  }
  acc = sa_wave_sum_d(acc);
  if (lane == 0) ws.e[(size_t)b * ws.F + t] = acc;
}

// grid B: the row's largest frame energy, then the kept frames' indices in ascending order, 256 frames a pass: a
// ballot gives every kept frame its slot, so each slot has one writer
__global__ __launch_bounds__(ST_THREADS) void sa_stoi_select_kernel(const int* __restrict__ n_valid, int N, StWs ws) {
  __shared__ double mx[ST_THREADS / 64];
  __shared__ int cnt[ST_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  const int F = st_frames(st_n10(st_nvalid(n_valid, b, N)));
  const double* e = ws.e + (size_t)b * ws.F;
  int* idx = ws.idx + (size_t)b * ws.F;
  double v = 0.0;
  for (int t = tid; t < F; t += ST_THREADS) v = fmax(v, e[t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if (lane == 0) mx[wv] = v;
  __syncthreads();
  const double thr = ST_RANGE * fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3]));
  int base = 0;
  for (int c0 = 0; c0 < F; c0 += ST_THREADS) {
    const int t = c0 + tid;
    const bool keep = t < F && e[t] > thr;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) cnt[wv] = __popcll(mask);
    __syncthreads();
    int off = base, all = 0;
#pragma unroll
    for (int w = 0; w < ST_THREADS / 64; ++w) {
      if (w < wv) off += cnt[w];
      all += cnt[w];
    }
    if (keep) idx[off + __popcll(mask & ((1ull << lane) - 1ull))] = t;
    base += all;
    __syncthreads();
  }
  if (tid == 0) ws.K[b] = base;
}

// grid (tiles of 8 compacted frames, B).  LDS: the twiddles (cos, sin)(pi i / 256), i < 512, as double2 (8 KiB), and
// the 16 windowed frames (8 of ref, 8 of deg) [16][256] fp64 (32 KiB), later the 16 x 212 powers.
//   fill   thread u forms sample u of every frame: consecutive doubles per wave, no bank conflict
//   DFT    thread i < 212 owns bin 7 + i for all 16 frames: the samples are read two at a time (ds_read_b128) from
//          one address per wave (a broadcast); the twiddle of (k n) mod 512 is one 16-byte read per sample, whose
//          addresses differ by 16 n bytes between neighbouring lanes -- conflict-free for odd n, up to a four-way
//          conflict at n = 128 -- against 32 fp64 FMAs per sample
//   bands  thread (v, j) adds its band's powers in bin order
__global__ __launch_bounds__(ST_THREADS) void sa_stoi_bands_kernel(StWs ws) {
  __shared__ double2 tw[ST_NFFT];
  __shared__ __attribute__((aligned(16))) double fr[2 * ST_FT * ST_W];
  const int tid = threadIdx.x, b = blockIdx.y, m0 = blockIdx.x * ST_FT;
  const int K = ws.K[b];
  if (m0 >= K) return;
  const int* idx = ws.idx + (size_t)b * ws.F;
  for (int i = tid; i < ST_NFFT; i += ST_THREADS) {
    double s, c;
    sincospi((double)i * (1.0 / 256.0), &s, &c);
    tw[i] = make_double2(c, s);
  }
  {
    const int u = tid;
    const double wu = st_window(u), wo = st_window(u ^ ST_H);
#pragma unroll
    for (int fi = 0; fi < ST_FT; ++fi) {
      const int m = m0 + fi;
      int t = 0, tn = -1;                                   // tn: the neighbour that overlaps this half, if any
      if (m < K) {
        t = idx[m];
        if (u < ST_H) { if (m >= 1) tn = idx[m - 1]; }
        else if (m + 1 < K) tn = idx[m + 1];
      }
#pragma unroll
      for (int sig = 0; sig < 2; ++sig) {
        const double* x = ws.x10 + ((size_t)b * 2 + sig) * ws.M;
        double a = 0.0;
        if (m < K) {
          a = wu * x[(size_t)ST_H * t + u];
          if (tn >= 0) a += wo * x[(size_t)ST_H * tn + (u ^ ST_H)];
        }
        fr[(sig * ST_FT + fi) * ST_W + u] = a * wu;
      }
    }
  }
  __syncthreads();
  double re[2 * ST_FT], im[2 * ST_FT];
#pragma unroll
  for (int v = 0; v < 2 * ST_FT; ++v) re[v] = 0.0, im[v] = 0.0;
  if (tid < ST_NK) {
    const int k = ST_K0 + tid;
    for (int n = 0; n < ST_W; n += 2) {
      const double2 t0 = tw[(k * n) & (ST_NFFT - 1)], t1 = tw[(k * (n + 1)) & (ST_NFFT - 1)];
#pragma unroll
      for (int v = 0; v < 2 * ST_FT; ++v) {
        const double2 s = *(const double2*)&fr[v * ST_W + n];
        re[v] = fma(s.x, t0.x, re[v]);
        im[v] = fma(s.x, t0.y, im[v]);
        re[v] = fma(s.y, t1.x, re[v]);
        im[v] = fma(s.y, t1.y, im[v]);
      }
    }
  }
  __syncthreads();
  if (tid < ST_NK) {
#pragma unroll
    for (int v = 0; v < 2 * ST_FT; ++v) fr[v * ST_NK + tid] = fma(re[v], re[v], im[v] * im[v]);
  }
  __syncthreads();
  if (tid < 2 * ST_FT * ST_NB) {
    const int v = tid / ST_NB, j = tid - ST_NB * v, sig = v / ST_FT, m = m0 + (v - ST_FT * sig);
    double acc = 0.0;
    for (int k = st_lo[j]; k < st_lo[j + 1]; ++k) acc += fr[v * ST_NK + k - ST_K0];
    if (m < K) ws.X[(((size_t)b * 2 + sig) * ST_NB + j) * ws.F + m] = sqrt(acc);
  }
}

__device__ static inline double st_gsum(double v) {         // over the 16 lanes of a segment, a fixed butterfly
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}

// grid (tiles of 16 segments, B): 16 lanes a segment, lane j < 15 band j (lane 15 carries zeros).  A lane holds its
// band's 30 magnitudes of X and Y in registers: the STOI correlation needs no other lane; the ESTOI column steps
// are 16-lane butterflies
__global__ __launch_bounds__(ST_THREADS) void sa_stoi_segments_kernel(StWs ws) {
  const int tid = threadIdx.x, j = tid & 15, b = blockIdx.y;
  const int s = blockIdx.x * ST_SG + (tid >> 4);
  const int K = ws.K[b], S = K >= ST_SEG ? K - ST_SEG + 1 : 0;
  if (blockIdx.x * ST_SG >= S) return;                      // (uniform)
  const bool live = s < S && j < ST_NB;
  double x[ST_SEG], y[ST_SEG];
  {
    const double* X = ws.X + (((size_t)b * 2) * ST_NB + j) * ws.F + s;
    const double* Y = X + (size_t)ST_NB * ws.F;
#pragma unroll
    for (int i = 0; i < ST_SEG; ++i) x[i] = live ? X[i] : 0.0, y[i] = live ? Y[i] : 0.0;
  }
  double sxx = 0.0, syy = 0.0, sx = 0.0, sy = 0.0;
#pragma unroll
  for (int i = 0; i < ST_SEG; ++i) sxx = fma(x[i], x[i], sxx), syy = fma(y[i], y[i], syy), sx += x[i], sy += y[i];
  const double alpha = sqrt(sxx) / (sqrt(syy) + ST_EPS);
  double sc = 0.0;
#pragma unroll
  for (int i = 0; i < ST_SEG; ++i) sc += fmin(alpha * y[i], ST_CLIP * x[i]);
  const double xm = sx / ST_SEG, ym = sy / ST_SEG, cm = sc / ST_SEG;
  double vx = 0.0, vy = 0.0, vc = 0.0;
#pragma unroll
  for (int i = 0; i < ST_SEG; ++i) {
    const double dx = x[i] - xm, dy = y[i] - ym, dc = fmin(alpha * y[i], ST_CLIP * x[i]) - cm;
    vx = fma(dx, dx, vx), vy = fma(dy, dy, vy), vc = fma(dc, dc, vc);
  }
  const double nx = sqrt(vx) + ST_EPS, ny = sqrt(vy) + ST_EPS, nc = sqrt(vc) + ST_EPS;
  double d = 0.0;
#pragma unroll
  for (int i = 0; i < ST_SEG; ++i) {
    const double c = (fmin(alpha * y[i], ST_CLIP * x[i]) - cm) / nc;
    x[i] = (x[i] - xm) / nx;                                // the rows, zero-mean and unit-norm along time
    y[i] = (y[i] - ym) / ny;
    d = fma(x[i], c, d);
  }
  const double stoi = st_gsum(d);
  double es = 0.0;
#pragma unroll
  for (int i = 0; i < ST_SEG; ++i) {                        // the columns, along the 15 bands
    const double mx = st_gsum(x[i]) / ST_NB, my = st_gsum(y[i]) / ST_NB;
    const double dx = j < ST_NB ? x[i] - mx : 0.0, dy = j < ST_NB ? y[i] - my : 0.0;
    const double cx = sqrt(st_gsum(dx * dx)) + ST_EPS, cy = sqrt(st_gsum(dy * dy)) + ST_EPS;
    es += st_gsum((dx / cx) * (dy / cy));
  }
  if (j == 0 && s < S) {
    double* o = ws.part + 2 * ((size_t)b * ws.F + s);
    o[0] = stoi;
    o[1] = es / ST_SEG;
  }
}

// grid B, one wave: lane l adds the segments l, l + 64, ... in order, the wave by butterfly
__global__ __launch_bounds__(64) void sa_stoi_final_kernel(StWs ws, float* __restrict__ stoi,
                                                           float* __restrict__ estoi, int* __restrict__ frames,
                                                           int* __restrict__ segments) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const int K = ws.K[b], S = K >= ST_SEG ? K - ST_SEG + 1 : 0;
  double a = 0.0, c = 0.0;
  for (int s = lane; s < S; s += 64) {
    a += ws.part[2 * ((size_t)b * ws.F + s)];
    c += ws.part[2 * ((size_t)b * ws.F + s) + 1];
  }
  a = sa_wave_sum_d(a), c = sa_wave_sum_d(c);
  if (lane == 0) {
    stoi[b] = S ? (float)(a / ((double)ST_NB * S)) : 0.0f;
    if (estoi) estoi[b] = S ? (float)(c / (double)S) : 0.0f;
    if (frames) frames[b] = K;
    if (segments) segments[b] = S;
  }
}

extern "C" int sa_stoi(const float* ref, const float* deg, const int* n_valid, int B, int N, const double* taps,
                       float* stoi, float* estoi, int* frames, int* segments, void* wsp, void* stream) {
  if (!ref || !deg || !n_valid || !taps || !stoi || !wsp || B < 1 || B > ST_MAX_B || N < 1 || N > ST_MAX_N)
    return -EINVAL;
  StWs ws;
  ws.M = (int)((5ll * N + 7) / 8);
  ws.F = ws.M >= ST_W ? (ws.M - ST_W) / ST_H + 1 : 1;
  ws.x10 = (double*)wsp;
  ws.e = ws.x10 + (size_t)B * 2 * ws.M;
  ws.X = ws.e + (size_t)B * ws.F;
  ws.part = ws.X + (size_t)B * 2 * ST_NB * ws.F;
  ws.idx = (int*)(ws.part + (size_t)B * 2 * ws.F);
  ws.K = ws.idx + (size_t)B * ws.F;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sa_stoi_resample_kernel, dim3(sa_div_up(ws.M, ST_THREADS), B, 2), dim3(ST_THREADS), 0, s, ref,
                     deg, n_valid, N, taps, ws);
  hipLaunchKernelGGL(sa_stoi_energy_kernel, dim3(sa_div_up(ws.F, ST_THREADS / 64), B), dim3(ST_THREADS), 0, s,
                     n_valid, N, ws);
  hipLaunchKernelGGL(sa_stoi_select_kernel, dim3(B), dim3(ST_THREADS), 0, s, n_valid, N, ws);
  hipLaunchKernelGGL(sa_stoi_bands_kernel, dim3(sa_div_up(ws.F, ST_FT), B), dim3(ST_THREADS), 0, s, ws);
  hipLaunchKernelGGL(sa_stoi_segments_kernel, dim3(sa_div_up(ws.F, ST_SG), B), dim3(ST_THREADS), 0, s, ws);
  hipLaunchKernelGGL(sa_stoi_final_kernel, dim3(B), dim3(64), 0, s, ws, stoi, estoi, frames, segments);
  return -(int)hipGetLastError();
}
