// Modulation-spectrum smoothing (include/sa_hip.h, "modulation-spectrum smoothing"): a symmetric
// FIR along time over every STFT bin's log magnitude, the input's phases kept.  Two launches behind one entry point:
//   sa_modspec_peak_kernel    per-workgroup partial maxima of re^2 + im^2 over the frames that count
//   sa_modspec_smooth_kernel  one workgroup per (MS_TT frames) x (MS_KB bins) tile: fp64 L of the tile and J frames
//                             either side staged in LDS, MS_FPT consecutive frames of one bin per thread
// All arithmetic is fp64 formed from the fp32 input; only the output rounds to fp32.  No atomics, fixed orders.
#include "sa_common.h"
#include <errno.h>

#define MS_NFFT 400
#define MS_HOP 160
#define MS_BINS 201
#define MS_JMAX 64
#define MS_TT 128                              // frames per workgroup
#define MS_KB 16                               // bins per workgroup
#define MS_FPT 8                               // consecutive frames per thread
#define MS_THREADS (MS_KB * (MS_TT / MS_FPT))  // 256
#define MS_ROWS (MS_TT + 2 * MS_JMAX)          // staged frames at the largest J
// doubles per staged frame: 8 * MS_PITCH = 144 = 16 (mod 32) doubles puts the bins of two neighbouring frame groups
// (the two halves of a 32-lane group of ds_read_b64) on the two halves of the 64 banks
#define MS_PITCH 18
#define MS_PK_MAX 256                          // partial maxima per row, at most
#define MS_PK_FRAMES 64                        // frames per partial maximum, at least
#define MS_PK_THREADS 256
#define MS_MAX_B 65535
#define MS_MAX_T (1 << 23)

static_assert(MS_THREADS == 256 && MS_TT % MS_FPT == 0, "one thread per (bin, group of MS_FPT frames)");
static_assert(MS_ROWS * MS_PITCH * 8 <= 64 * 1024, "the staged tile is one workgroup's LDS");
static_assert(MS_FPT == 8, "the register windows below rotate modulo 8");

extern "C" int sa_modspec_dim(int which) {
  switch (which) {
    case 0: return MS_NFFT;
    case 1: return MS_HOP;
    case 2: return MS_BINS;
    case 3: return MS_JMAX;
    case 4: return MS_TT;
    case 5: return MS_KB;
    case 6: return MS_FPT;
    case 7: return MS_PK_MAX;
    case 8: return MS_PK_FRAMES;
    default: return -EINVAL;
  }
}

static inline int ms_chunks(int T) {
  const int n = sa_div_up(T, MS_PK_FRAMES);
  return n < MS_PK_MAX ? n : MS_PK_MAX;
}

extern "C" long long sa_modspec_workspace_bytes(int B, int T) {
  if (B < 1 || B > MS_MAX_B || T < 1 || T > MS_MAX_T) return -EINVAL;
  return 8LL * B * ms_chunks(T);
}

__device__ static inline int ms_frames(const int* __restrict__ frames, int b, int T) {
  const int f = frames[b];
  return f < 0 ? 0 : (f > T ? T : f);
}

// re^2 + im^2 in fp64: both products are exact (24 x 24 bits), the sum rounds once (fused or not)
__device__ static inline double ms_power(float2 v) {
  const double re = (double)v.x, im = (double)v.y;
  return re * re + im * im;
}

// ---- stage 1: partial[b][c] = max of re^2 + im^2 over the frames [c F, min((c + 1) F, T_b)) and all bins ----
__global__ __launch_bounds__(MS_PK_THREADS) void sa_modspec_peak_kernel(const float2* __restrict__ R,
                                                                        const int* __restrict__ frames, int T, int F,
                                                                        double* __restrict__ partial) {
  __shared__ double wmax[MS_PK_THREADS / SA_WAVE];
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int Tb = ms_frames(frames, b, T);
  const long long lo = (long long)c * F;
  long long hi = lo + F;
  if (hi > Tb) hi = Tb;
  const float2* row = R + (long long)b * T * MS_BINS;
  double m = 0.0;
  for (long long i = lo * MS_BINS + tid; i < hi * MS_BINS; i += MS_PK_THREADS) m = fmax(m, ms_power(row[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if ((tid & (SA_WAVE - 1)) == 0) wmax[tid / SA_WAVE] = m;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < MS_PK_THREADS / SA_WAVE; ++w) m = fmax(m, wmax[w]);
    partial[(long long)b * gridDim.x + c] = m;
  }
}

// ---- stage 2: the smoothing pass ----
__global__ __launch_bounds__(MS_THREADS) void sa_modspec_smooth_kernel(
    const float2* __restrict__ R, const double* __restrict__ taps, int J, const float* __restrict__ depth,
    const int* __restrict__ frames, int T, float floor_rel, float max_gain_ln, const double* __restrict__ partial,
    int nch, float2* __restrict__ C, double* __restrict__ peak, double* __restrict__ Lout) {
  __shared__ double Ls[MS_ROWS * MS_PITCH];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int t0 = blockIdx.x * MS_TT, k0 = blockIdx.y * MS_KB;
  const int Tb = ms_frames(frames, b, T);
  const float dv = depth[b];
  const double d = dv > 0.0f ? (dv < 1.0f ? (double)dv : 1.0) : 0.0;      // a NaN compares false: 0
  const long long base = (long long)b * T * MS_BINS;

  // the row's peak, from the partial maxima (exact in any order; every workgroup of the row forms the same value)
  double pk = 0.0;
  for (int c = 0; c < nch; ++c) pk = fmax(pk, partial[(long long)b * nch + c]);
  pk = __dsqrt_rn(pk);
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) peak[b] = pk;

  const int kq = tid & (MS_KB - 1), k = k0 + kq;        // this thread's bin
  const int grp = tid / MS_KB;                           // its group of frames, and its row when staging
  const int tend = t0 + MS_TT < T ? t0 + MS_TT : T;      // the tile's frames are [t0, tend)

  // nothing of this tile is transformed: copy it (and clear Lout past T_b; a row with depth 0 still reports L)
  const bool live = t0 < Tb && (d != 0.0 || Lout != nullptr);
  if (!live) {
    if (k < MS_BINS) {
      for (int t = t0 + grp; t < tend; t += MS_THREADS / MS_KB) {
        const long long i = base + (long long)t * MS_BINS + k;
        C[i] = R[i];
        if (Lout != nullptr) Lout[i] = 0.0;
      }
    }
    return;
  }

  // stage L of the frames c(t0 - J) .. c(t0 + MS_TT - 1 + J): staged row r holds frame clamp(t0 - J + r, 0, T_b - 1)
  const double fl = fmax((double)floor_rel * pk, 1e-10);
  const int rows = MS_TT + 2 * J;
  for (int r = grp; r < rows; r += MS_THREADS / MS_KB) {
    int t = t0 - J + r;
    t = t < 0 ? 0 : (t > Tb - 1 ? Tb - 1 : t);
    double L = 0.0;
    if (k < MS_BINS) L = log(fmax(__dsqrt_rn(ms_power(R[base + (long long)t * MS_BINS + k])), fl));
    Ls[r * MS_PITCH + kq] = L;
  }
  __syncthreads();
  if (k >= MS_BINS) return;

  // MS_FPT consecutive frames of one bin: the windows lo[o] = L[t - j], hi[o] = L[t + j] slide by one staged value
  // a step, so each j costs two LDS reads for MS_FPT outputs.  Output o's lo sits in slot (o - j) mod 8 and its hi in
  // slot (o + j) mod 8; the loop is unrolled by 8 so that every slot is a register.
  const int u0 = grp * MS_FPT;                            // first frame of this thread within the tile
  const double* col = Ls + (u0 + J) * MS_PITCH + kq;      // staged L of frame t0 + u0
  double ctr[MS_FPT], lo[MS_FPT], hi[MS_FPT], acc[MS_FPT];
  const double h0 = taps[0];
#pragma unroll
  for (int o = 0; o < MS_FPT; ++o) {
    ctr[o] = lo[o] = hi[o] = col[o * MS_PITCH];
    acc[o] = h0 * ctr[o];
  }
  for (int j0 = 1; j0 <= J; j0 += MS_FPT) {
#pragma unroll
    for (int jj = 0; jj < MS_FPT; ++jj) {
      const int j = j0 + jj;
      if (j <= J) {
        lo[(7 - jj) & 7] = col[-j * MS_PITCH];
        hi[jj & 7] = col[(MS_FPT - 1 + j) * MS_PITCH];
        const double hj = taps[j];
#pragma unroll
        for (int o = 0; o < MS_FPT; ++o) acc[o] = fma(hj, lo[(o - jj - 1) & 7] + hi[(o + jj + 1) & 7], acc[o]);
      }
    }
  }

  const double gmax = (double)max_gain_ln;
#pragma unroll
  for (int o = 0; o < MS_FPT; ++o) {
    const int t = t0 + u0 + o;
    if (t < tend) {
      const long long i = base + (long long)t * MS_BINS + k;
      const float2 v = R[i];
      if (t < Tb) {
        double g = d * (acc[o] - ctr[o]);
        g = fmin(fmax(g, -gmax), gmax);
        if (d != 0.0) {
          const double e = exp(g);
          C[i] = make_float2((float)((double)v.x * e), (float)((double)v.y * e));
        } else {
          C[i] = v;
        }
        if (Lout != nullptr) Lout[i] = ctr[o] + g;
      } else {
        C[i] = v;
        if (Lout != nullptr) Lout[i] = 0.0;
      }
    }
  }
}

extern "C" int sa_modspec_smooth(const void* R, const double* taps, int J, const float* depth, const int* frames,
                                 int B, int T, float floor_rel, float max_gain_ln, void* C, double* peak, double* Lout,
                                 void* ws, void* stream) {
  if (!R || !taps || !depth || !frames || !C || !peak || !ws || C == R) return -EINVAL;
  if (B < 1 || B > MS_MAX_B || T < 1 || T > MS_MAX_T || J < 0 || J > MS_JMAX) return -EINVAL;
  if (!(floor_rel > 0.0f && floor_rel < 1.0f) || !(max_gain_ln > 0.0f)) return -EINVAL;
  const int nch = ms_chunks(T), F = sa_div_up(T, nch);
  hipLaunchKernelGGL(sa_modspec_peak_kernel, dim3(nch, B), dim3(MS_PK_THREADS), 0, (hipStream_t)stream,
                     (const float2*)R, frames, T, F, (double*)ws);
  hipLaunchKernelGGL(sa_modspec_smooth_kernel, dim3(sa_div_up(T, MS_TT), sa_div_up(MS_BINS, MS_KB), B),
                     dim3(MS_THREADS), 0, (hipStream_t)stream, (const float2*)R, taps, J, depth, frames, T, floor_rel,
                     max_gain_ln, (const double*)ws, nch, (float2*)C, peak, Lout);
  return -(int)hipGetLastError();
}
