// SpecAugment of the ConvAE train step's input features (specaug.py): bicubic time warp, frequency
// masks and time masks of speechbrain 0.5.x lobes/augment.py::SpecAugment, restated.  x, out [B][T][F] fp32, F a
// multiple of 4 up to 128.  Three launches per step:
//   sa_specaug_warp_sums  out = the warped rows (four taps along time); per workgroup the fp64 sum of its values
//                         and of those in frequency-masked columns
//   sa_specaug_finalize   the two fill values from the partial sums (fp64, fixed order, rounded once)
//   sa_specaug_fill       stores the fill values on masked cells; reads no activations
// Every random draw is made on the host and arrives in one plan buffer (layout: specaug.py): the warp centre, the
// tables and the masks are data, so the launch parameters depend on (B, T, F) alone.
#include "sa_common.h"
#include <errno.h>

#define SPA_TILE 32                        // output frames per workgroup
#define SPA_THREADS 256
#define SPA_WAVES (SPA_THREADS / SA_WAVE)
#define SPA_HEADER 8                       // flags, B, T, F, reserved
#define SPA_ROW_WORDS 8                    // base, lo, hi, 0, four weights
#define SPA_MAX_MASKS 8
#define SPA_PAIR_WORDS (2 * SPA_MAX_MASKS)
#define SPA_MAX_F 128
#define SPA_FLAG_ZERO 1

__device__ static inline const int* spa_rows(const int* plan) { return plan + SPA_HEADER; }
__device__ static inline const int* spa_freq(const int* plan, int B, int T) {
  return plan + SPA_HEADER + SPA_ROW_WORDS * T;
}
__device__ static inline const int* spa_time(const int* plan, int B, int T) {
  return spa_freq(plan, B, T) + SPA_PAIR_WORDS * B;
}
__device__ static inline const int* spa_nfm(const int* plan, int B, int T) {
  return spa_time(plan, B, T) + SPA_PAIR_WORDS * B;
}

// 1 if position p lies in one of the utterance's (pos, len) pairs
__device__ static inline int spa_masked(const int* __restrict__ pairs, int p) {
  int m = 0;
#pragma unroll
  for (int k = 0; k < SPA_MAX_MASKS; ++k) {
    const int pos = pairs[2 * k], len = pairs[2 * k + 1];
    m |= (p >= pos) & (p - pos < len);
  }
  return m;
}

// ---- warp + sums -----------------------------------------------------------------------------------------
// grid (tiles of SPA_TILE output frames, B).  The tile's rows are contiguous in out: thread i takes the 16-byte
// quads i, i + 256, ... of the tile, so a wave writes 1 KiB runs; the four source rows of a quad are 16-byte
// loads too (neighbouring output rows share them through L2).  Sums: every thread adds its values in fp64 in
// quad order, the wave adds its lanes by butterfly, thread 0 adds the four waves in order: no atomics, the
// same bits on every run.
__global__ __launch_bounds__(SPA_THREADS) void sa_specaug_warp_sums_kernel(const float* __restrict__ x,
                                                                           const int* __restrict__ plan, int B, int T,
                                                                           int F, float* __restrict__ out,
                                                                           double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) int rows[SPA_TILE * SPA_ROW_WORDS];
  __shared__ __attribute__((aligned(4))) unsigned char colm[SPA_MAX_F];
  __shared__ double red[2 * SPA_WAVES];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * SPA_TILE;
  const int nrows = min(SPA_TILE, T - t0), Q = F >> 2;

  if (tid < nrows * SPA_ROW_WORDS) rows[tid] = spa_rows(plan)[(size_t)t0 * SPA_ROW_WORDS + tid];
  if (tid < F) colm[tid] = (unsigned char)spa_masked(spa_freq(plan, B, T) + SPA_PAIR_WORDS * b, tid);
  __syncthreads();

  const float4* xb = reinterpret_cast<const float4*>(x + (size_t)b * T * F);
  float4* ob = reinterpret_cast<float4*>(out + ((size_t)b * T + t0) * F);
  double s_all = 0.0, s_fm = 0.0;
  for (int i = tid; i < nrows * Q; i += SPA_THREADS) {
    const int r = i / Q, q = i - r * Q;
    const int* e = rows + r * SPA_ROW_WORDS;
    const int base = e[0], lo = max(e[1], 0), hi = min(e[2], T - 1);      // (whatever the plan holds: inside x)
    const float w0 = __int_as_float(e[4]), w1 = __int_as_float(e[5]), w2 = __int_as_float(e[6]),
                w3 = __int_as_float(e[7]);
    const float4 a0 = xb[(size_t)min(max(base - 1, lo), hi) * Q + q];
    const float4 a1 = xb[(size_t)min(max(base, lo), hi) * Q + q];
    const float4 a2 = xb[(size_t)min(max(base + 1, lo), hi) * Q + q];
    const float4 a3 = xb[(size_t)min(max(base + 2, lo), hi) * Q + q];
    float4 v;
    v.x = fmaf(w3, a3.x, fmaf(w2, a2.x, fmaf(w1, a1.x, w0 * a0.x)));
    v.y = fmaf(w3, a3.y, fmaf(w2, a2.y, fmaf(w1, a1.y, w0 * a0.y)));
    v.z = fmaf(w3, a3.z, fmaf(w2, a2.z, fmaf(w1, a1.z, w0 * a0.z)));
    v.w = fmaf(w3, a3.w, fmaf(w2, a2.w, fmaf(w1, a1.w, w0 * a0.w)));
    ob[i] = v;
    const unsigned m = reinterpret_cast<const unsigned*>(colm)[q];
    s_all += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    s_fm += ((m & 0x1u ? (double)v.x : 0.0) + (m & 0x100u ? (double)v.y : 0.0)) +
            ((m & 0x10000u ? (double)v.z : 0.0) + (m & 0x1000000u ? (double)v.w : 0.0));
  }
  s_all = sa_wave_sum_d(s_all);
  s_fm = sa_wave_sum_d(s_fm);
  if ((tid & (SA_WAVE - 1)) == 0) {
    red[2 * (tid >> 6)] = s_all;
    red[2 * (tid >> 6) + 1] = s_fm;
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, f = 0.0;
    for (int w = 0; w < SPA_WAVES; ++w) {
      a += red[2 * w];
      f += red[2 * w + 1];
    }
    const size_t p = (size_t)b * gridDim.x + blockIdx.x;
    part[2 * p] = a;
    part[2 * p + 1] = f;
  }
}

// ---- the fill values -------------------------------------------------------------------------------------
// one workgroup: thread i adds the partial pairs i, i + 256, ... in index order, the wave adds its lanes by
// butterfly, thread 0 the four waves in order (fp64; the order depends on npart alone).  n_fm is an integer sum.
//   val_f = S / N                                   (the mean of the warped tensor)
//   val_t = (S - S_fm + n_fm val_f) / N             (the mean after the frequency masks; val_f as stored)
// both rounded once to fp32; 0 with replace_with_zero
__global__ __launch_bounds__(SPA_THREADS) void sa_specaug_finalize_kernel(const double* __restrict__ part, int npart,
                                                                          const int* __restrict__ plan, int B, int T,
                                                                          int F, float* __restrict__ vals) {
  __shared__ double red[3 * SPA_WAVES];
  const int tid = threadIdx.x;
  double a = 0.0, f = 0.0, n = 0.0;
  for (int i = tid; i < npart; i += SPA_THREADS) {
    a += part[2 * (size_t)i];
    f += part[2 * (size_t)i + 1];
  }
  const int* nfm = spa_nfm(plan, B, T);
  for (int i = tid; i < B; i += SPA_THREADS) n += (double)nfm[i];      // integers under 2^53: exact in any order
  a = sa_wave_sum_d(a);
  f = sa_wave_sum_d(f);
  n = sa_wave_sum_d(n);
  if ((tid & (SA_WAVE - 1)) == 0) {
    red[3 * (tid >> 6)] = a;
    red[3 * (tid >> 6) + 1] = f;
    red[3 * (tid >> 6) + 2] = n;
  }
  __syncthreads();
  if (tid == 0) {
    double S = 0.0, Sf = 0.0, nf = 0.0;
    for (int w = 0; w < SPA_WAVES; ++w) {
      S += red[3 * w];
      Sf += red[3 * w + 1];
      nf += red[3 * w + 2];
    }
    float vf = 0.0f, vt = 0.0f;
    if (!(plan[0] & SPA_FLAG_ZERO)) {
      const double N = (double)B * (double)T * (double)F;
      vf = (float)(S / N);
      vt = (float)((S - Sf + nf * (double)vf) / N);
    }
    vals[0] = vf;
    vals[1] = vt;
  }
}

// ---- the masks -------------------------------------------------------------------------------------------
// the grid of sa_specaug_warp_sums.  A time-masked row gets val_t whatever its columns; elsewhere the
// frequency-masked columns get val_f.  Workgroups whose tile has no masked cell return after the flags.
__global__ __launch_bounds__(SPA_THREADS) void sa_specaug_fill_kernel(const int* __restrict__ plan,
                                                                      const float* __restrict__ vals, int B, int T,
                                                                      int F, float* __restrict__ out) {
  __shared__ __attribute__((aligned(4))) unsigned char colm[SPA_MAX_F];
  __shared__ unsigned char rowm[SPA_TILE];
  __shared__ int any;
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * SPA_TILE;
  const int nrows = min(SPA_TILE, T - t0), Q = F >> 2;
  if (tid == 0) any = 0;
  __syncthreads();
  int mine = 0;
  if (tid < F) mine = colm[tid] = (unsigned char)spa_masked(spa_freq(plan, B, T) + SPA_PAIR_WORDS * b, tid);
  if (tid >= SPA_MAX_F && tid < SPA_MAX_F + nrows)
    mine = rowm[tid - SPA_MAX_F] =
        (unsigned char)spa_masked(spa_time(plan, B, T) + SPA_PAIR_WORDS * b, t0 + tid - SPA_MAX_F);
  if (mine) any = 1;                       // (every writer stores the same value)
  __syncthreads();
  if (!any) return;

  const float vf = vals[0], vt = vals[1];
  float* ob = out + ((size_t)b * T + t0) * F;
  for (int i = tid; i < nrows * Q; i += SPA_THREADS) {
    const int r = i / Q, q = i - r * Q;
    float* o = ob + 4 * (size_t)i;
    if (rowm[r]) {
      *reinterpret_cast<float4*>(o) = make_float4(vt, vt, vt, vt);
      continue;
    }
    const unsigned m = reinterpret_cast<const unsigned*>(colm)[q];
    if (m == 0x01010101u) {
      *reinterpret_cast<float4*>(o) = make_float4(vf, vf, vf, vf);
    } else if (m) {
      if (m & 0x1u) o[0] = vf;
      if (m & 0x100u) o[1] = vf;
      if (m & 0x10000u) o[2] = vf;
      if (m & 0x1000000u) o[3] = vf;
    }
  }
}

static int spa_bad_shape(int B, int T, int F) {
  return B < 1 || B > 65535 || T < 1 || F < 4 || (F & 3) || F > SPA_MAX_F;
}
static int spa_unaligned(const void* p) { return (int)((uintptr_t)p & 15); }

extern "C" int sa_specaug_warp_sums(const float* x, const void* plan, int B, int T, int F, float* out, double* part,
                                    void* stream) {
  if (!x || !plan || !out || !part || x == out || spa_bad_shape(B, T, F) || spa_unaligned(x) || spa_unaligned(out))
    return -EINVAL;
  hipLaunchKernelGGL(sa_specaug_warp_sums_kernel, dim3(sa_div_up(T, SPA_TILE), B), dim3(SPA_THREADS), 0,
                     (hipStream_t)stream, x, (const int*)plan, B, T, F, out, part);
  return -(int)hipGetLastError();
}

extern "C" int sa_specaug_finalize(const double* part, const void* plan, int B, int T, int F, float* vals,
                                   void* stream) {
  if (!part || !plan || !vals || spa_bad_shape(B, T, F)) return -EINVAL;
  hipLaunchKernelGGL(sa_specaug_finalize_kernel, dim3(1), dim3(SPA_THREADS), 0, (hipStream_t)stream, part,
                     sa_div_up(T, SPA_TILE) * B, (const int*)plan, B, T, F, vals);
  return -(int)hipGetLastError();
}

extern "C" int sa_specaug_fill(const void* plan, const float* vals, int B, int T, int F, float* out, void* stream) {
  if (!plan || !vals || !out || spa_bad_shape(B, T, F) || spa_unaligned(out)) return -EINVAL;
  hipLaunchKernelGGL(sa_specaug_fill_kernel, dim3(sa_div_up(T, SPA_TILE), B), dim3(SPA_THREADS), 0,
                     (hipStream_t)stream, (const int*)plan, vals, B, T, F, out);
  return -(int)hipGetLastError();
}
