// Griffin-Lim inversion of the front end's features (vocoder.py): normalised log-Mel frames
// back to a waveform.  n_fft 400, hop 160, 201 bins, the periodic Hamming window of features.py, center=True with
// zero padding: T frames <-> N = (T - 1) 160 samples.  Three kernels:
//   sa_mel_to_mag  S = sqrt(max(0, p M)), p = 10^((x std + mean) / 10), M the filterbank's pseudo-inverse
//   sa_gl_istft    y = overlap-add of the windowed inverse real DFTs of C over the window envelope
//   sa_gl_project  R = STFT(y); A = R - m Tprev; C' = S A / (|A| + 1e-16)
// The loop is {sa_gl_istft, sa_gl_project} n_iter times and one more sa_gl_istft.  Both transforms are the dense
// real DFT in fp32 FMAs.  The twiddles are a table of cos and sin(2 pi i / 400), i = 0..399, made in fp64 and
// rounded once, read at the integer (k j) mod 400, which a thread steps by addition.  A thread owns one index q
// in 0..100 of the OUTPUT side and keeps, per frame, four sums -- cosine and sine terms over the even and over
// the odd indices of the summed side -- because the tables' symmetries give a second output from the same sums
// (cos((200 - q) i) = (-1)^i cos(q i), sin((200 - q) i) = -(-1)^i sin(q i)), and in the inverse, where the output
// runs to 399, a third and fourth (cos((400 - q) i) = cos(q i), sin((400 - q) i) = -sin(q i)): a quarter (inverse)
// or half (forward) of the dense form's multiplications.  The frames' operands lie interleaved in LDS, so one
// 16-byte broadcast read feeds four FMAs.  No atomics: the overlap-add gathers.
#include "sa_common.h"
#include <errno.h>

#define GL_NFFT 400
#define GL_HOP 160
#define GL_NBIN 201
#define GL_G 8                         // hop blocks (sa_gl_istft) or frames (sa_gl_project) per workgroup
#define GL_F (GL_G + 2)                // frames that touch GL_G hop blocks
#define GL_THREADS 128                 // 101 of them own an output index
#define GL_MAX_B 65535                 // grid.y
#define GL_MAX_T (1 << 23)             // 160 T + 400 stays an int
#define MM_FRAMES 16                   // frames per workgroup of sa_mel_to_mag
#define MM_THREADS 256
#define MM_MELS 80

extern "C" int sa_gl_tile(void) { return GL_G; }

static inline bool gl_shape_ok(int B, int T, int least) {    // rows, and frames (at least `least` of them)
  return B >= 1 && B <= GL_MAX_B && T >= least && T <= GL_MAX_T;
}

// ---- Mel -> linear magnitude ---------------------------------------------------------------------------
// grid (tiles of 16 frames, B).  The tile's powers p[m][f] are formed once (the affine in fp64, so the exponent's
// argument is rounded once) and held in LDS; thread k < 201 then runs the 80-term dot product of every frame with
// column k of M, whose loads are contiguous over the lanes.  Frames t >= T of x are never read.
__global__ __launch_bounds__(MM_THREADS) void sa_mel_to_mag_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ mean,
                                                                   const float* __restrict__ stdv,
                                                                   const float* __restrict__ M, int T, int Tf,
                                                                   float* __restrict__ S) {
  __shared__ __attribute__((aligned(16))) float p[MM_MELS][MM_FRAMES];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * MM_FRAMES;
  for (int i = tid; i < MM_MELS * MM_FRAMES; i += MM_THREADS) {
    const int f = i / MM_MELS, m = i - f * MM_MELS;
    float v = 0.0f;
    if (t0 + f < T) {
      const double db = (double)x[((size_t)b * Tf + t0 + f) * MM_MELS + m] * (double)stdv[m] + (double)mean[m];
      v = exp2f((float)(db * 0.33219280948873623));          // log2(10) / 10
    }
    p[m][f] = v;
  }
  __syncthreads();
  if (tid >= GL_NBIN) return;
  float acc[MM_FRAMES];
#pragma unroll
  for (int f = 0; f < MM_FRAMES; ++f) acc[f] = 0.0f;
#pragma unroll 4
  for (int m = 0; m < MM_MELS; ++m) {
    const float mv = M[m * GL_NBIN + tid];
#pragma unroll
    for (int q = 0; q < MM_FRAMES / 4; ++q) {
      const float4 pv = *reinterpret_cast<const float4*>(&p[m][4 * q]);
      acc[4 * q + 0] = fmaf(pv.x, mv, acc[4 * q + 0]);
      acc[4 * q + 1] = fmaf(pv.y, mv, acc[4 * q + 1]);
      acc[4 * q + 2] = fmaf(pv.z, mv, acc[4 * q + 2]);
      acc[4 * q + 3] = fmaf(pv.w, mv, acc[4 * q + 3]);
    }
  }
#pragma unroll
  for (int f = 0; f < MM_FRAMES; ++f)
    if (t0 + f < T) S[((size_t)b * T + t0 + f) * GL_NBIN + tid] = sqrtf(fmaxf(acc[f], 0.0f));
}

extern "C" int sa_mel_to_mag(const float* x, const float* mean, const float* stdv, const float* M, int B, int T,
                             int Tf, float* S, void* stream) {
  if (!x || !mean || !stdv || !M || !S || !gl_shape_ok(B, T, 1) || T > Tf) return -EINVAL;
  hipLaunchKernelGGL(sa_mel_to_mag_kernel, dim3(sa_div_up(T, MM_FRAMES), B), dim3(MM_THREADS), 0,
                     (hipStream_t)stream, x, mean, stdv, M, T, Tf, S);
  return -(int)hipGetLastError();
}

// ---- inverse STFT -----------------------------------------------------------------------------------------
// grid (tiles of GL_G hop blocks, B).  In padded coordinates p = n + 200 the samples [0, N) lie in the hop blocks
// h = 1..T; block h is touched by the frames h - 2, h - 1, h.  A workgroup owns the blocks h0..h0 + 7 and
//   1. stages the 201 bins of its 10 frames as coef[k][f] = (c_k Re C, -c_k Im C), c = 1 at k = 0 and 200 (whose
//      imaginary parts do not enter), else 2; zeros for frames outside [0, T)
//   2. thread q <= 100: the four sums per frame over k, then x[q], x[200 + q], x[400 - q], x[200 - q], each times
//      w / 400, into xs[f][j]
//   3. every sample of the tile: the sum of its 2 or 3 frames' xs over the sum of their w^2
// One k of step 2: the ten frames' staged pairs of row k times the twiddles at idx = (k tid) mod 400, added to the
// cosine sums cs and the sine sums sn (the even k's or the odd k's); idx steps on to the next k.
__device__ static inline void gl_istft_step(const float* coef_k, const float* tcos, const float* tsin, int tid,
                                            int& idx, float (&cs)[GL_F], float (&sn)[GL_F]) {
  const float c = tcos[idx], s = tsin[idx];
  const float4* row = reinterpret_cast<const float4*>(coef_k);
#pragma unroll
  for (int v = 0; v < GL_F / 2; ++v) {
    const float4 a = row[v];
    cs[2 * v] = fmaf(a.x, c, cs[2 * v]);
    sn[2 * v] = fmaf(a.y, s, sn[2 * v]);
    cs[2 * v + 1] = fmaf(a.z, c, cs[2 * v + 1]);
    sn[2 * v + 1] = fmaf(a.w, s, sn[2 * v + 1]);
  }
  idx += tid;
  if (idx >= GL_NFFT) idx -= GL_NFFT;
}

__global__ __launch_bounds__(GL_THREADS) void sa_gl_istft_kernel(const float2* __restrict__ C,
                                                                 const float* __restrict__ win,
                                                                 const float* __restrict__ tw, int T,
                                                                 float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float coef[GL_NBIN][2 * GL_F];
  __shared__ float xs[GL_F][GL_NFFT];
  __shared__ float tcos[GL_NFFT], tsin[GL_NFFT], wl[GL_NFFT];
  const int tid = threadIdx.x, b = blockIdx.y, h0 = 1 + blockIdx.x * GL_G, tf0 = h0 - 2;
  const int N = (T - 1) * GL_HOP;

  for (int i = tid; i < GL_NFFT; i += GL_THREADS) {
    tcos[i] = tw[i];
    tsin[i] = tw[GL_NFFT + i];
    wl[i] = win[i];
  }
  for (int i = tid; i < GL_F * GL_NBIN; i += GL_THREADS) {
    const int f = i / GL_NBIN, k = i - f * GL_NBIN, t = tf0 + f;
    float2 c = make_float2(0.0f, 0.0f);
    if (t >= 0 && t < T) c = C[((size_t)b * T + t) * GL_NBIN + k];
    const bool edge = k == 0 || k == GL_NFFT / 2;
    coef[k][2 * f] = edge ? c.x : 2.0f * c.x;
    coef[k][2 * f + 1] = edge ? 0.0f : -2.0f * c.y;
  }
  __syncthreads();

  if (tid <= 100) {
    float ce[GL_F], se[GL_F], co[GL_F], so[GL_F];
#pragma unroll
    for (int f = 0; f < GL_F; ++f) ce[f] = se[f] = co[f] = so[f] = 0.0f;
    int idx = 0;                                   // (k tid) mod 400
#pragma unroll 1
    for (int k = 0; k < GL_NBIN; k += 2) {
      gl_istft_step(coef[k], tcos, tsin, tid, idx, ce, se);
      if (k + 1 < GL_NBIN) gl_istft_step(coef[k + 1], tcos, tsin, tid, idx, co, so);
    }
    const float inv = 1.0f / GL_NFFT;
    const bool twin = tid > 0 && tid < 100;        // 400 - q and 200 - q are further samples
#pragma unroll
    for (int f = 0; f < GL_F; ++f) {
      const float cp = ce[f] + co[f], cm = ce[f] - co[f], sp = se[f] + so[f], sm = se[f] - so[f];
      xs[f][tid] = (cp + sp) * inv * wl[tid];
      xs[f][200 + tid] = (cm + sm) * inv * wl[200 + tid];
      if (twin) {
        xs[f][400 - tid] = (cp - sp) * inv * wl[400 - tid];
        xs[f][200 - tid] = (cm - sm) * inv * wl[200 - tid];
      }
    }
  }
  __syncthreads();

  for (int o = tid; o < GL_G * GL_HOP; o += GL_THREADS) {
    const int p = h0 * GL_HOP + o, n = p - GL_NFFT / 2;
    if (n < 0 || n >= N) continue;
    const int hb = o / GL_HOP, r = o - hb * GL_HOP;
    float acc = 0.0f, env = 0.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int f = hb + 2 - d, j = r + d * GL_HOP, t = tf0 + f;      // frame h0 + hb - d
      if (j < GL_NFFT && t >= 0 && t < T) {
        acc += xs[f][j];
        env = fmaf(wl[j], wl[j], env);
      }
    }
    y[(size_t)b * N + n] = acc / env;
  }
}

extern "C" int sa_gl_istft(const void* C, const float* window, const float* twiddle, int B, int T, float* y,
                           void* stream) {
  if (!C || !window || !twiddle || !y || !gl_shape_ok(B, T, 2)) return -EINVAL;
  hipLaunchKernelGGL(sa_gl_istft_kernel, dim3(sa_div_up(T, GL_G), B), dim3(GL_THREADS), 0, (hipStream_t)stream,
                     (const float2*)C, window, twiddle, T, y);
  return -(int)hipGetLastError();
}

// ---- projection and phase update ------------------------------------------------------------------------------
// grid (tiles of GL_G frames, B).  A workgroup
//   1. stages z[j][f] = w[j] ypad[160 (t0 + f) + j] of its 8 frames (zeros outside [0, N) and for frames >= T)
//   2. thread q <= 100: the four sums per frame over j, then R[q] and R[200 - q]
//   3. the update of those bins, in fp64 from the fp32 R, Tprev, S and m (201 of them per frame against the
//      transform's 400 x 201 FMAs): A = R - m Tprev; C' = S A / (|A| + 1e-16), rounded once; stores C' and R
// One j of step 2: the eight frames' staged samples of row j times the twiddles at idx = (tid j) mod 400, added to the
// cosine sums cs and the sine sums sn (the even j's or the odd j's); idx steps on to the next j.
__device__ static inline void gl_project_step(const float* z_j, const float* tcos, const float* tsin, int tid,
                                              int& idx, float (&cs)[GL_G], float (&sn)[GL_G]) {
  const float c = tcos[idx], s = tsin[idx];
  const float4* row = reinterpret_cast<const float4*>(z_j);
#pragma unroll
  for (int v = 0; v < GL_G / 4; ++v) {
    const float4 a = row[v];
    cs[4 * v] = fmaf(a.x, c, cs[4 * v]);
    sn[4 * v] = fmaf(a.x, s, sn[4 * v]);
    cs[4 * v + 1] = fmaf(a.y, c, cs[4 * v + 1]);
    sn[4 * v + 1] = fmaf(a.y, s, sn[4 * v + 1]);
    cs[4 * v + 2] = fmaf(a.z, c, cs[4 * v + 2]);
    sn[4 * v + 2] = fmaf(a.z, s, sn[4 * v + 2]);
    cs[4 * v + 3] = fmaf(a.w, c, cs[4 * v + 3]);
    sn[4 * v + 3] = fmaf(a.w, s, sn[4 * v + 3]);
  }
  idx += tid;
  if (idx >= GL_NFFT) idx -= GL_NFFT;
}

__global__ __launch_bounds__(GL_THREADS) void sa_gl_project_kernel(const float* __restrict__ y,
                                                                   const float* __restrict__ S,
                                                                   const float2* __restrict__ Tprev, float mom,
                                                                   const float* __restrict__ win,
                                                                   const float* __restrict__ tw, int T,
                                                                   float2* __restrict__ Cn, float2* __restrict__ R) {
  __shared__ __attribute__((aligned(16))) float z[GL_NFFT][GL_G];
  __shared__ float tcos[GL_NFFT], tsin[GL_NFFT];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * GL_G;
  const int N = (T - 1) * GL_HOP;

  for (int i = tid; i < GL_NFFT; i += GL_THREADS) {
    tcos[i] = tw[i];
    tsin[i] = tw[GL_NFFT + i];
  }
  for (int i = tid; i < GL_G * GL_NFFT; i += GL_THREADS) {
    const int f = i / GL_NFFT, j = i - f * GL_NFFT;
    const int n = (t0 + f) * GL_HOP + j - GL_NFFT / 2;
    float v = 0.0f;
    if (t0 + f < T && n >= 0 && n < N) v = win[j] * y[(size_t)b * N + n];
    z[j][f] = v;
  }
  __syncthreads();
  if (tid > 100) return;

  float ce[GL_G], se[GL_G], co[GL_G], so[GL_G];
#pragma unroll
  for (int f = 0; f < GL_G; ++f) ce[f] = se[f] = co[f] = so[f] = 0.0f;
  int idx = 0;                                     // (tid j) mod 400
#pragma unroll 1
  for (int j = 0; j < GL_NFFT; j += 2) {
    gl_project_step(z[j], tcos, tsin, tid, idx, ce, se);
    gl_project_step(z[j + 1], tcos, tsin, tid, idx, co, so);
  }

  const double m = (double)mom;
#pragma unroll
  for (int f = 0; f < GL_G; ++f) {
    if (t0 + f >= T) break;
    const size_t base = ((size_t)b * T + t0 + f) * GL_NBIN;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      if (side && tid == 100) continue;            // 200 - 100 is bin 100 again
      const int k = side ? GL_NFFT / 2 - tid : tid;
      const float re = side ? ce[f] - co[f] : ce[f] + co[f];
      const float im = side ? se[f] - so[f] : -(se[f] + so[f]);
      const float2 tp = Tprev[base + k];
      const double ar = (double)re - m * (double)tp.x, ai = (double)im - m * (double)tp.y;
      const double g = (double)S[base + k] / (sqrt(ar * ar + ai * ai) + 1e-16);
      R[base + k] = make_float2(re, im);
      Cn[base + k] = make_float2((float)(g * ar), (float)(g * ai));
    }
  }
}

extern "C" int sa_gl_project(const float* y, const float* S, const void* Tprev, float momentum_ratio,
                             const float* window, const float* twiddle, int B, int T, void* C_new, void* R,
                             void* stream) {
  if (!y || !S || !Tprev || !window || !twiddle || !C_new || !R || !gl_shape_ok(B, T, 2)) return -EINVAL;
  hipLaunchKernelGGL(sa_gl_project_kernel, dim3(sa_div_up(T, GL_G), B), dim3(GL_THREADS), 0, (hipStream_t)stream,
                     y, S, (const float2*)Tprev, momentum_ratio, window, twiddle, T, (float2*)C_new, (float2*)R);
  return -(int)hipGetLastError();
}
