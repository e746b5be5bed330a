// Waveform augmentation of the gender-classifier recipes (augment.py): additive noise rows
// (the env_corrupt analogue), speed perturbation (Kaldi-style windowed-sinc resampling), frequency drop (a
// 101-tap filter composed of notches on the host) and chunk drop, restated from speechbrain 0.5.x
// processing/speech_augmentation.py.  Three launches per step:
//   sa_wav_abs_sums  per-row sum |x| of the waveforms and of the noise (fp64, fixed order)
//   sa_noise_scales  (1 - f_b, g_b) per utterance, formed in fp64 on the device
//   sa_wav_augment   noise mix, resampling, filter and chunk drop in one read and one write of the waveform
// Every random draw but the noise tensor is made on the host and arrives in one plan buffer (layout: augment.py).
#include "sa_common.h"
#include <errno.h>

#define AUG_TILE 2048                      // output samples per workgroup
#define AUG_HALO 50                        // (taps - 1) / 2
#define AUG_TAPS 101
#define AUG_THREADS 256
#define AUG_RS (AUG_TILE + 2 * AUG_HALO)   // resampled samples a tile's filter reads
#define AUG_XS_MAX 3072                    // staged input samples (speeds down to ~72 %)
#define AUG_WT_MAX 2048                    // S_out * W
#define AUG_PH_MAX 128                     // S_out
#define AUG_W_MAX 32
#define AUG_MAX_CHUNKS 8                   // dropped intervals per row
#define AUG_CHUNK_STRIDE (1 + 2 * AUG_MAX_CHUNKS)

// ---- per-row sum |x| ---------------------------------------------------------------------------------
// grid (B, 1 | 2): one workgroup per row of wav (y = 0) or noise (y = 1).  Every thread adds its strided
// elements in fp64, the wave adds its lanes by butterfly, thread 0 adds the 16 waves in order: no atomics,
// the same bits on every run.
__global__ __launch_bounds__(1024) void sa_wav_abs_sums_kernel(const float* __restrict__ wav,
                                                               const float* __restrict__ noise, int L,
                                                               double* __restrict__ sums) {
  __shared__ double part[16];
  const int tid = threadIdx.x, b = blockIdx.x, B = gridDim.x, which = blockIdx.y;
  const float* p = (which ? noise : wav) + (size_t)b * L;
  double acc = 0.0;
  int head = (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3);      // scalars up to 16-byte alignment
  if (head > L) head = L;
  if (tid < head) acc += (double)fabsf(p[tid]);
  const int nv = (L - head) >> 2;
  const float4* pv = reinterpret_cast<const float4*>(p + head);
  for (int i = tid; i < nv; i += 4096) {                      // four independent 16-byte loads in flight
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = i + 1024 * u;
      v[u] = k < nv ? pv[k] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      acc += (double)fabsf(v[u].x) + (double)fabsf(v[u].y) + (double)fabsf(v[u].z) + (double)fabsf(v[u].w);
  }
  const int tail = head + 4 * nv;
  if (tid < L - tail) acc += (double)fabsf(p[tail + tid]);
  acc = sa_wave_sum_d(acc);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < 16; ++w) s += part[w];
    sums[(size_t)which * B + b] = s;
  }
}

extern "C" int sa_wav_abs_sums(const float* wav, const float* noise, int B, int L, double* sums, void* stream) {
  if (!wav || !sums || B < 1 || B > 65535 || L < 1) return -EINVAL;
  hipLaunchKernelGGL(sa_wav_abs_sums_kernel, dim3(B, noise ? 2 : 1), dim3(1024), 0, (hipStream_t)stream, wav, noise,
                     L, sums);
  return -(int)hipGetLastError();
}

// ---- noise scales ------------------------------------------------------------------------------------
// amp = sum |x| / (lens L); f = 1 / (10^(snr / 20) + 1); scales[b] = (1 - f, f amp_clean / (amp_noise + 1e-14)):
// fp64 throughout, rounded once to fp32
__global__ void sa_noise_scales_kernel(const double* __restrict__ sums, const float* __restrict__ lens,
                                       const float* __restrict__ snr, int B, int L, float* __restrict__ scales) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double den = (double)lens[b] * (double)L;
  const double ac = sums[b] / den, an = sums[B + b] / den;
  const double f = 1.0 / (pow(10.0, (double)snr[b] / 20.0) + 1.0);
  scales[2 * b] = (float)(1.0 - f);
  scales[2 * b + 1] = (float)(f * ac / (an + 1e-14));
}

extern "C" int sa_noise_scales(const double* sums, const float* lens, const float* snr, int B, int L,
                               float* scales, void* stream) {
  if (!sums || !lens || !snr || !scales || B < 1 || L < 1) return -EINVAL;
  hipLaunchKernelGGL(sa_noise_scales_kernel, dim3(sa_div_up(B, 64)), dim3(64), 0, (hipStream_t)stream, sums, lens,
                     snr, B, L, scales);
  return -(int)hipGetLastError();
}

// ---- the fused pass ----------------------------------------------------------------------------------
// grid (tiles of AUG_TILE output samples, R rows).  Row r < B is utterance r as it is; row B + b is
// c0 wav[b] + c1 noise[b] with (c0, c1) = scales[b], formed while the input span is staged.
//   1. xs: the input samples the tile's resampled span needs, zeros outside [0, L)
//   2. rs: resampled samples n in [t0 - 50, t0 + TILE + 50), n = q S_out + i -> sum_j w[i][j] x[q S_in + first[i] + j],
//      zeros outside [0, Lp)
//   3. y[n] = sum_j h[j] rs[n + j - 50]: a thread makes 4 consecutive outputs per pass from 26 16-byte LDS reads
//      (lane stride 16 bytes: the 16 lanes of a ds_read_b128 group cover the 64 banks once), every value read
//      once and used by up to 4 accumulators; the taps are wave-uniform loads
//   4. the row's chunk intervals zero their samples; store
__global__ __launch_bounds__(AUG_THREADS) void sa_wav_augment_kernel(
    const float* __restrict__ wav, const float* __restrict__ noise, const float* __restrict__ scales,
    const int* __restrict__ first, const float* __restrict__ w, const float* __restrict__ h,
    const int* __restrict__ chunks, int B, int L, int Lp, int S_in, int S_out, int W, int first_min,
    int first_max, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float rs[AUG_RS];
  __shared__ float xs[AUG_XS_MAX];
  __shared__ float wt[AUG_WT_MAX];
  __shared__ int fi[AUG_PH_MAX];
  const int tid = threadIdx.x, row = blockIdx.y, t0 = blockIdx.x * AUG_TILE;
  const bool noisy = row >= B;
  const int b = noisy ? row - B : row;
  const float c0 = noisy ? scales[2 * b] : 1.0f, c1 = noisy ? scales[2 * b + 1] : 0.0f;

  for (int p = tid; p < S_out * W; p += AUG_THREADS) wt[p] = w[p];
  for (int p = tid; p < S_out; p += AUG_THREADS) fi[p] = first[p];

  const int n_lo = max(t0 - AUG_HALO, 0), n_hi = min(t0 + AUG_TILE + AUG_HALO, Lp) - 1;
  const int in_lo = (n_lo / S_out) * S_in + first_min;
  const int span = min((n_hi / S_out) * S_in + first_max + W - in_lo, AUG_XS_MAX);
  const float* xr = wav + (size_t)b * L;
  const float* nr = noisy ? noise + (size_t)b * L : nullptr;
  for (int p = tid; p < span; p += AUG_THREADS) {
    const int k = in_lo + p;
    float v = 0.0f;
    if (k >= 0 && k < L) {
      v = xr[k];
      if (noisy) v = fmaf(c1, nr[k], c0 * v);
    }
    xs[p] = v;
  }
  __syncthreads();

  for (int p = tid; p < AUG_RS; p += AUG_THREADS) {
    const int n = t0 - AUG_HALO + p;
    float r = 0.0f;
    if (n >= 0 && n < Lp) {
      const int q = n / S_out, i = n - q * S_out;
      const int base = q * S_in + fi[i] - in_lo;
      const float* wr = wt + i * W;
      for (int j = 0; j < W; ++j) {
        const int idx = base + j;
        const float xv = (unsigned)idx < (unsigned)span ? xs[idx] : 0.0f;
        r = fmaf(wr[j], xv, r);
      }
    }
    rs[p] = r;
  }
  __syncthreads();

  const int* ck = chunks + (size_t)row * AUG_CHUNK_STRIDE;
  const int nck = min(ck[0], AUG_MAX_CHUNKS);
  float* orow = out + (size_t)row * Lp;
  const bool vec = (Lp & 3) == 0;          // rows of a multiple of 4 samples stay 16-byte aligned
#pragma unroll 1
  for (int pass = 0; pass < AUG_TILE / (4 * AUG_THREADS); ++pass) {
    const int o = pass * 4 * AUG_THREADS + 4 * tid;
    if (t0 + o >= Lp) continue;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int v = 0; v < (AUG_TAPS + 3 + 3) / 4; ++v) {
      const float4 q4 = *reinterpret_cast<const float4*>(&rs[o + 4 * v]);
      const float qv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = 4 * v + e - k;
          if (j >= 0 && j < AUG_TAPS) acc[k] = fmaf(h[j], qv[e], acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int n = t0 + o + k;
      for (int c = 0; c < nck; ++c)
        if (n >= ck[1 + 2 * c] && n < ck[2 + 2 * c]) acc[k] = 0.0f;
    }
    if (vec) {
      *reinterpret_cast<float4*>(&orow[t0 + o]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (t0 + o + k < Lp) orow[t0 + o + k] = acc[k];
    }
  }
}

extern "C" int sa_wav_augment_tile(void) { return AUG_TILE; }
extern "C" int sa_wav_augment_max_chunks(void) { return AUG_MAX_CHUNKS; }

// plan: 32-bit words in device memory -- first[S_out] (int), w[S_out][W], h[101] (float),
// chunks[R][1 + 2 * max_chunks] (int: count, then start, end pairs)
extern "C" int sa_wav_augment(const float* wav, const float* noise, const float* scales, const void* plan, int B,
                              int L, int R, int Lp, int S_in, int S_out, int W, int first_min, int first_max,
                              float* out, void* stream) {
  if (!wav || !plan || !out || B < 1 || L < 1 || Lp < 1 || (R != B && R != 2 * B) || R > 65535) return -EINVAL;
  if (R == 2 * B && (!noise || !scales)) return -EINVAL;
  if (S_in < 1 || S_out < 1 || S_out > AUG_PH_MAX || W < 1 || W > AUG_W_MAX || S_out * W > AUG_WT_MAX ||
      first_min > first_max)
    return -EINVAL;
  // the widest input span of a tile: whole periods under AUG_RS outputs, one more at each end, the phases' reach
  const long long span = ((long long)(AUG_RS - 1) / S_out + 2) * S_in + (first_max - first_min) + W;
  if (span > AUG_XS_MAX) return -EINVAL;
  const int* first = (const int*)plan;
  const float* w = (const float*)plan + S_out;
  const float* h = w + S_out * W;
  const int* chunks = first + S_out + S_out * W + AUG_TAPS;
  hipLaunchKernelGGL(sa_wav_augment_kernel, dim3(sa_div_up(Lp, AUG_TILE), R), dim3(AUG_THREADS), 0,
                     (hipStream_t)stream, wav, noise, scales, first, w, h, chunks, B, L, Lp, S_in, S_out, W,
                     first_min, first_max, out);
  return -(int)hipGetLastError();
}
